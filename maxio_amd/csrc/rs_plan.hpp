// rs_plan.hpp — host side of every Reed-Solomon launch: which launches a call
// becomes (rs_plan_mixed) and the descriptor tables of each (RsTable), for
// the uniform, grouped and multi-r forms alike.  All of it is arithmetic on
// pointers and sizes; no pointer is dereferenced.
//
// Host-only (no HIP, no I/O): ops.cpp runs it over a DescWriter,
// tools/kernel_lab over an RsImage, and tests/c_manifest/rs_plan_check.cpp
// on its own under -fsanitize=address,undefined.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "locate_plan.hpp"
#include "rs_args.hpp"

namespace mxec {

// One object of an RS launch: k inputs -> r outputs, device pointers.
struct RsObject {
    const uint8_t* const* in;  // k
    const uint64_t* in_len;    // k
    uint8_t* const* out;       // r
    const uint64_t* out_len;   // r
    uint32_t coef_off;         // dword offset of this object's [j][i][8] table
    // Verify (ReedSolomon::verify) when set, for every object of the call or
    // none: `out` are the stored parity rows, read and compared with the
    // recomputed ones, never written; first_bad (device, r entries, filled
    // with 0xFF on the stream ahead of the call) receives per row the lowest
    // byte offset at which they differ (rs_args.hpp RsArgs::first_bad).
    uint64_t* first_bad = nullptr;
    // Locate (mxec_locate) when set instead, again for every object of the
    // call or none: the verify's launch with r = m in 2..8 rows, but a
    // mismatch is classified and folded into this device record (a
    // LocateRec, rs_args.hpp; initialised with launch_locate_init on the
    // stream ahead of the call).  The launch uploads the (k, m) tables of
    // locate_plan.hpp with its descriptor tables.
    void* locate = nullptr;
    // Seeded store (uniform launches only, every object of the call or none):
    // r rows the accumulators start from instead of zero, read below out_len
    // like the rows written; never the rows of `out` (RsArgs::seed_ptrs).
    const uint8_t* const* seed = nullptr;
};

// An object of a mixed batch: its own k and shard size.
struct RsMixedObject {
    int k;
    uint64_t shard_size;
    RsObject o;
};

// Whether every pointer of the object is 16-byte aligned (the fast kernels'
// condition; the edge kernel takes the others).
inline bool rs_aligned(const RsObject& ob, int k, int r) {
    uintptr_t bits = 0;
    for (int j = 0; j < k; ++j) bits |= reinterpret_cast<uintptr_t>(ob.in[j]);
    for (int i = 0; i < r; ++i) bits |= reinterpret_cast<uintptr_t>(ob.out[i]);
    for (int i = 0; i < r && ob.seed; ++i) bits |= reinterpret_cast<uintptr_t>(ob.seed[i]);
    return (bits & 15) == 0;
}

enum RsPass : int { kRsStore = 0, kRsVerify = 1, kRsLocate = 2 };
inline RsPass rs_pass_of(const RsObject& ob) {
    return ob.locate ? kRsLocate : ob.first_bad ? kRsVerify : kRsStore;
}

// The descriptor tables of one launch.  The caller says what the launch is
// (the first block of fields), lay() reserves the sections in a writer --
// anything with add(bytes) -> offset, each section rounded up to 16 bytes and
// zero-filled, and data() -> base once every add is done -- put() fills one
// object after another, and args() turns the offsets into an RsArgs over the
// uploaded copy.
struct RsTable {
    uint64_t n_obj = 0, n_in = 0;  // objects, and input entries (the sum of their k)
    uint32_t r = 0;                // output entries per object: r_total; kMultiR under multi
    uint64_t tile = 0;             // bytes of a shard per tile
    bool tiled = false;            // grouped: one RsTileRec per tile
    bool multi = false;            //   ... with k | r << 16 in the record
    bool aligned = true;           // uniform: false sends every tile to the edge list
    uint64_t n_list = 0;           // tile records (tiled) or edge entries (unaligned), else 0
    RsPass pass = kRsStore;
    bool seeded = false;           // uniform store: a seed row per output entry (set before lay)
    std::map<int, uint32_t> loc_of_k;  // locate: k -> byte offset of its (k, r) table within o_lt

    size_t o_in = 0, o_out = 0, o_inlen = 0, o_outlen = 0, o_coef = 0, o_list = 0, o_res = 0;
    size_t o_lf = 0, o_lt = 0, o_lo = 0;  // locate: field block, (k, r) tables, each object's offset
    size_t o_seed = 0;                    // seeded: [n_obj][r] seed rows, behind every other section
    uint64_t o = 0, in0 = 0, t0 = 0;      // put()'s next object, input entry and list entry

    // Objects of any k and shard size: n_in input entries and n_tiles tiles
    // in all, r rows each (multi: r = kMultiR, each object's own in its records).
    static RsTable grouped(uint64_t n, uint64_t n_in, uint64_t n_tiles, uint32_t r, uint64_t tile, RsPass pass,
                           bool multi = false) {
        RsTable t;
        t.n_obj = n, t.n_in = n_in, t.r = r, t.tile = tile, t.n_list = n_tiles, t.pass = pass;
        t.tiled = true, t.multi = multi;
        return t;
    }
    // n objects of one (k, r, shard_size); unaligned: every tile in the edge list.
    static RsTable uniform(uint64_t n, int k, int r, uint64_t shard_size, uint64_t tile, bool aligned, RsPass pass) {
        const uint64_t n_edge = aligned ? 0 : n * ((shard_size + tile - 1) / tile);
        RsTable t = grouped(n, n * uint64_t(k), n_edge, uint32_t(r), tile, pass);
        t.tiled = false, t.aligned = aligned;
        return t;
    }

    // Locate: an object of this k is coming (before lay).
    void locate_k(int k) {
        const uint32_t at = uint32_t(loc_of_k.size()) * locate_table_bytes(int(r));
        loc_of_k.emplace(k, at);
    }

    // own_field: the launch carries the field block itself (a uniform launch);
    // grouped launches share one, which their caller adds last and names in
    // every table's o_lf.
    template <class W>
    void lay(W& w, bool own_field) {
        o_in = w.add(sizeof(void*) * n_in);
        o_out = w.add(sizeof(void*) * n_obj * r);
        o_inlen = w.add(8 * n_in);
        o_outlen = w.add(8 * n_obj * r);  // zero: unused output entries (multi)
        o_coef = w.add(4 * n_obj);
        o_list = w.add((tiled ? sizeof(RsTileRec) : 8) * n_list);
        if (pass != kRsStore) o_res = w.add(sizeof(void*) * n_obj);
        if (seeded) o_seed = w.add(sizeof(void*) * n_obj * r);
        if (pass != kRsLocate) return;
        if (own_field) o_lf = w.add(kLocateFieldBytes);
        o_lt = w.add(loc_of_k.size() * locate_table_bytes(int(r)));
        o_lo = w.add(4 * n_obj);
    }

    // The next object: k inputs, r_obj outputs (r, or the object's own under
    // multi), lengths clamped to its shard size.
    void put(char* hb, const RsObject& ob, int k, int r_obj, uint64_t shard_size) {
        const uint64_t obj = o++, first = in0, nt = (shard_size + tile - 1) / tile;
        auto** ip = reinterpret_cast<const uint8_t**>(hb + o_in) + first;
        auto* il = reinterpret_cast<uint64_t*>(hb + o_inlen) + first;
        auto** op = reinterpret_cast<uint8_t**>(hb + o_out) + obj * r;
        auto* ol = reinterpret_cast<uint64_t*>(hb + o_outlen) + obj * r;
        for (int j = 0; j < k; ++j) {
            ip[j] = ob.in[j];
            il[j] = std::min<uint64_t>(ob.in_len[j], shard_size);
        }
        for (int i = 0; i < r_obj; ++i) {
            op[i] = ob.out[i];
            ol[i] = std::min<uint64_t>(ob.out_len[i], shard_size);
        }
        reinterpret_cast<uint32_t*>(hb + o_coef)[obj] = ob.coef_off;
        if (seeded)
            for (int i = 0; i < r_obj; ++i) (reinterpret_cast<const uint8_t**>(hb + o_seed) + obj * r)[i] = ob.seed[i];
        if (pass != kRsStore)
            reinterpret_cast<void**>(hb + o_res)[obj] = pass == kRsLocate ? ob.locate : static_cast<void*>(ob.first_bad);
        if (pass == kRsLocate) reinterpret_cast<uint32_t*>(hb + o_lo)[obj] = loc_of_k.at(k);
        in0 = first + uint64_t(k);
        if (tiled) {
            auto* tr = reinterpret_cast<RsTileRec*>(hb + o_list) + t0;
            const uint32_t kr = uint32_t(k) | (multi ? uint32_t(r_obj) << 16 : 0u);
            for (uint64_t t = 0; t < nt; ++t) tr[t] = RsTileRec{uint32_t(obj), kr, uint32_t(first), uint32_t(t)};
        } else if (!aligned) {
            auto* ed = reinterpret_cast<uint64_t*>(hb + o_list) + t0;
            for (uint64_t t = 0; t < nt; ++t) ed[t] = obj << 32 | t;
        }
        t0 += nt;
    }

    // The launch over the uploaded tables at db.  Left to the caller: coef,
    // the grid fields, a uniform launch's k and shard_size and its row blocks
    // (r, row0).
    RsArgs args(char* db) const {
        RsArgs a{};
        a.in_ptrs = reinterpret_cast<const uint8_t* const*>(db + o_in);
        a.out_ptrs = reinterpret_cast<uint8_t* const*>(db + o_out);
        a.in_len = reinterpret_cast<const uint64_t*>(db + o_inlen);
        a.out_len = reinterpret_cast<const uint64_t*>(db + o_outlen);
        a.coef_off = reinterpret_cast<const uint32_t*>(db + o_coef);
        a.n_obj = uint32_t(n_obj);
        a.r = a.r_total = r;
        a.aligned = aligned ? 1u : 0u;
        if (tiled) {
            a.tiles = reinterpret_cast<const RsTileRec*>(db + o_list);
            a.n_tiles = n_list;
            a.multi = multi ? 1u : 0u;
        } else {
            a.edge_list = reinterpret_cast<const uint64_t*>(db + o_list);
            a.n_edge = n_list;
            a.edge_tile_bytes = tile;
        }
        if (pass == kRsLocate) {
            a.locate = reinterpret_cast<LocateRec* const*>(db + o_res);
            a.loc_field = reinterpret_cast<const uint8_t*>(db + o_lf);
            a.loc_tab = reinterpret_cast<const uint8_t*>(db + o_lt);
            a.loc_off = reinterpret_cast<const uint32_t*>(db + o_lo);
        } else if (pass == kRsVerify) {
            a.first_bad = reinterpret_cast<uint64_t* const*>(db + o_res);
        }
        if (seeded) a.seed_ptrs = reinterpret_cast<const uint8_t* const*>(db + o_seed);
        return a;
    }
};

// The locate tables of n launches laid out in one image: the field block
// once (t[0].o_lf) and every launch's (k, r) tables, each from
// table(k, r, out) -> status (the encoding matrix lives with the caller).
template <class F>
int rs_locate_fill(char* hb, const RsTable* t, size_t n, F&& table) {
    locate_field_tables(reinterpret_cast<uint8_t*>(hb + t[0].o_lf));
    for (size_t i = 0; i < n; ++i)
        for (const auto& kt : t[i].loc_of_k)
            if (const int rc = table(kt.first, int(t[i].r), reinterpret_cast<uint8_t*>(hb + t[i].o_lt + kt.second))) return rc;
    return 0;
}

// The plainest writer: a host image (tools/kernel_lab, the stand-alone check).
struct RsImage {
    std::vector<char> v;
    size_t add(size_t bytes) {
        const size_t off = v.size();
        v.resize(off + ((bytes + 15) & ~size_t(15)), 0);
        return off;
    }
    char* data() { return v.data(); }
};

// What a mixed call (objects grouped by r) becomes.
struct RsMixedPlan {
    struct Group {  // one grouped launch
        int r = 0;
        std::vector<RsMixedObject> objs;
        uint64_t sum_k = 0, n_tiles = 0, tile = 0;
    };
    struct Rest {  // one uniform launch (run_rs)
        int r = 0, k = 0;
        uint64_t shard_size = 0;
        std::vector<RsObject> objs;
    };
    std::vector<Group> grouped;
    std::vector<Rest> rest;  // per r in map order, within r by first appearance of (k, shard_size)
    bool multi = false;      // the grouped launches run as one multi-r launch ...
    uint64_t m_obj = 0, m_k = 0, m_tiles = 0;  // ... of these totals
};

// Per r, the objects whose pointers are all 16-byte aligned (r <= 8) take one
// grouped launch if their index ranges fit its 32-bit fields; a call that is
// one uniform aligned group keeps the uniform kernel (no tile table).  The
// others -- per r the unaligned ones, then a group that did not qualify --
// take one uniform launch per (k, shard_size), whose edge kernel takes
// unaligned pointers.  Two or more grouped launches, all of r <= kMultiR and
// the multi-r tile, within that launch's limits: one multi-r launch instead,
// never for a verify or a locate (`checked`), which run one launch per r.
// tile_of(r): the grouped kernel's tile bytes for r rows.
template <class TileOf>
RsMixedPlan rs_plan_mixed(const std::map<int, std::vector<RsMixedObject>>& groups, TileOf&& tile_of,
                          uint64_t multi_tile, bool multi_on, bool checked) {
    RsMixedPlan p;
    auto to_rest = [&p](int r, const std::vector<RsMixedObject>& v) {
        std::map<std::pair<int, uint64_t>, size_t> at;
        for (const RsMixedObject& ob : v) {
            const auto it = at.emplace(std::make_pair(ob.k, ob.shard_size), p.rest.size());
            if (it.second) p.rest.push_back({r, ob.k, ob.shard_size, {}});
            p.rest[it.first->second].objs.push_back(ob.o);
        }
    };
    for (const auto& g : groups) {
        const int r = g.first;
        if (g.second.empty() || r == 0) continue;
        RsMixedPlan::Group al;
        std::vector<RsMixedObject> un;
        for (const RsMixedObject& ob : g.second) (r <= 8 && rs_aligned(ob.o, ob.k, r) ? al.objs : un).push_back(ob);
        to_rest(r, un);
        if (al.objs.empty()) continue;
        bool uniform = true;
        al.r = r;
        al.tile = tile_of(r);
        for (const RsMixedObject& ob : al.objs) {
            uniform &= ob.k == al.objs[0].k && ob.shard_size == al.objs[0].shard_size;
            al.sum_k += uint64_t(ob.k);
            al.n_tiles += (ob.shard_size + al.tile - 1) / al.tile;
        }
        const bool fits =
            al.objs.size() <= UINT32_MAX && al.sum_k <= UINT32_MAX && al.n_tiles <= (uint64_t(1) << 32);
        if (fits && !(uniform && groups.size() == 1 && un.empty())) p.grouped.push_back(std::move(al));
        else to_rest(r, al.objs);
    }
    p.multi = multi_on && !checked && p.grouped.size() >= 2;
    for (const RsMixedPlan::Group& g : p.grouped) {
        p.multi = p.multi && g.r <= int(kMultiR) && g.tile == multi_tile;
        p.m_obj += g.objs.size();
        p.m_k += g.sum_k;
        p.m_tiles += g.n_tiles;
    }
    p.multi = p.multi && p.m_obj <= UINT32_MAX / kMultiR && p.m_k <= UINT32_MAX && p.m_tiles <= (uint64_t(1) << 32);
    return p;
}

}  // namespace mxec
