// decode_tables.hpp — host side of every reconstruct's decode launch: from
// each object's decode plan, the `in` / `in_len` / `out` / `out_len` tables
// and the objects grouped by number of rebuilt shards, as run_rs_mixed takes
// them (rs_plan.hpp).  Shard addresses are arithmetic only; no device pointer
// is dereferenced.
//
// Host-only (no HIP, no I/O): ops.cpp's decode_step runs it under every
// reconstruct, and tests/c_manifest/decode_tables_check.cpp on its own under
// -fsanitize=address,undefined.
#pragma once

#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include "gf256.hpp"
#include "rs_plan.hpp"

namespace mxec {

// One object of a decode: k + m shards of S bytes on the device.
struct DecodeItem {
    int k, m;
    uint64_t S;
    const uint64_t* len;   // k + m, clamped to S
    uint8_t* present;      // k + m flags (host): decode_step's plan lookup reads them, the tables never
    uint8_t* const* ptrs;  // shard i at ptrs[i], or (null) ...
    uint8_t* base;         // ... at base + i * stride
    uint64_t stride;
    const DecodePlan* plan = nullptr;  // null: none (short of k shards, or it ends before the window)
    uint32_t coef_off = 0;             // dword offset of the plan's coefficient table
    uint8_t* shard(int i) const { return ptrs ? ptrs[i] : base + uint64_t(i) * stride; }
};

// The four tables of one launch and the RsObjects over them.
struct DecodeTables {
    std::vector<const uint8_t*> in;
    std::vector<uint8_t*> out;
    std::vector<uint64_t> in_len, out_len;

    // Bytes [off, off + pw) of every item's `missing` shards from the same
    // bytes of its `valid` ones, in plan order (RS is bytewise): every
    // pointer advanced by off, every length L > off ? min(pw, L - off) : 0,
    // the shard size min(pw, S - off); the caller gives an item with S <= off
    // no plan.  An item without a plan, or with nothing missing, contributes
    // nothing.  Keyed by missing.size().  The tables are sized up front (the
    // RsObjects point into them) and stand until the next build.
    std::map<int, std::vector<RsMixedObject>> build(const std::vector<DecodeItem>& items, uint64_t off = 0,
                                                    uint64_t pw = ~uint64_t(0)) {
        size_t n_in = 0, n_out = 0;
        for (const DecodeItem& it : items)
            if (it.plan && !it.plan->missing.empty()) {
                n_in += size_t(it.k);
                n_out += it.plan->missing.size();
            }
        in.assign(n_in, nullptr);
        out.assign(n_out, nullptr);
        in_len.assign(n_in, 0);
        out_len.assign(n_out, 0);
        std::map<int, std::vector<RsMixedObject>> groups;
        size_t pi = 0, po = 0;
        for (const DecodeItem& it : items) {
            if (!it.plan || it.plan->missing.empty()) continue;
            const DecodePlan& p = *it.plan;
            const int r = int(p.missing.size());
            auto window = [&](int i) { return it.len[i] > off ? std::min(pw, it.len[i] - off) : uint64_t(0); };
            for (int v = 0; v < it.k; ++v) {
                in[pi + v] = it.shard(p.valid[size_t(v)]) + off;
                in_len[pi + v] = window(p.valid[size_t(v)]);
            }
            for (int e = 0; e < r; ++e) {
                out[po + e] = it.shard(p.missing[size_t(e)]) + off;
                out_len[po + e] = window(p.missing[size_t(e)]);
            }
            groups[r].push_back(RsMixedObject{it.k, std::min(pw, it.S - off),
                                              RsObject{&in[pi], &in_len[pi], &out[po], &out_len[po], it.coef_off}});
            pi += size_t(it.k);
            po += size_t(r);
        }
        return groups;
    }
};

}  // namespace mxec
