// ops.cpp — kernel launches over device pointers: the RS launches planned by
// rs_plan.hpp, the grid tuner, the coefficient lookups, the SHA-256 launches.
#include <cstdlib>

#include "ops.hpp"

#include <algorithm>
#include <climits>
#include <cstring>
#include <map>

#include "kernels.hpp"
#include "sha_plan.hpp"

namespace mxec {

int too_many_shards(uint64_t k, uint64_t m) {
    return set_error(MXEC_E_TOO_MANY_SHARDS_255,
                     "too many shards: " + std::to_string(k) + " data + " + std::to_string(m) + " parity = " +
                         std::to_string(k + m) + " > 255 (GF(2^8) limit). Increase --chunk-size");
}

int check_km(int k, int m) {
    if (k + m > 255) return too_many_shards(uint64_t(k), uint64_t(m));
    int rc = rs_check(k, m);
    if (rc) return set_error(rc, std::string("Reed-Solomon init error: ") + mxec_strerror(rc));
    return MXEC_OK;
}

int reconstruct_shape(int k, int m, uint64_t shard_size) {
    if (int rc = rs_check(k, m)) return set_error(rc, std::string("RS init error: ") + mxec_strerror(rc));
    if (shard_size == 0) return set_error(MXEC_E_EMPTY_SHARD, mxec_strerror(MXEC_E_EMPTY_SHARD));
    return MXEC_OK;
}

int encode_coef(Device& dev, int k, int m, uint32_t* off) {
    std::vector<uint8_t> key = {'E', uint8_t(k), uint8_t(m)};
    {
        std::lock_guard<std::mutex> g(dev.coef_mu);
        auto it = dev.coef_index.find(key);
        if (it != dev.coef_index.end()) {
            *off = it->second.off;
            coef_note_use(it->second.gen, it->second.seq);
            return MXEC_OK;
        }
    }
    auto mat = rs_matrix(k, m);
    if (!mat) return set_error(MXEC_E_SINGULAR_MATRIX, "encoding matrix construction failed");
    GfMatrix rows(m, k);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < k; ++j) rows.at(i, j) = mat->at(k + i, j);
    return coef_offset(dev, key, coef_tables(rows), off);
}

int decode_coef(Device& dev, const DecodePlan& plan, bool data_only, uint32_t* off) {
    std::vector<uint8_t> key = {'D', uint8_t(plan.k), uint8_t(plan.m), uint8_t(data_only)};
    for (int v : plan.valid) key.push_back(uint8_t(v));
    key.push_back(0xFF);
    for (int v : plan.missing) key.push_back(uint8_t(v));
    return coef_offset(dev, key, plan.table, off);
}

int decode_plan(Device& dev, int k, int m, const uint8_t* present, bool data_only,
                std::shared_ptr<const DecodePlan>* plan, uint32_t* off) {
    const int total = k + m;
    Device::PatternKey key;
    key.kmf = uint32_t(k) | uint32_t(m) << 8 | uint32_t(data_only) << 16;
    int np = 0;
    for (int i = 0; i < total; ++i) {
        const bool p = present[i] != 0;
        np += p;
        key.mask[size_t(i >> 6)] |= uint64_t(p) << (i & 63);
    }
    plan->reset();
    *off = 0;
    if (np < k) return MXEC_OK;
    {
        std::lock_guard<std::mutex> g(dev.coef_mu);
        auto it = dev.patterns.find(key);
        if (it != dev.patterns.end()) {
            *plan = std::static_pointer_cast<const DecodePlan>(it->second.plan);
            *off = it->second.off;
            if (!(*plan)->missing.empty()) coef_note_use(it->second.gen, it->second.seq);
            return MXEC_OK;
        }
    }
    auto p = decode_cache().get(k, m, present, data_only);
    if (!p) return set_error(MXEC_E_SINGULAR_MATRIX, "decode matrix inversion failed");
    uint32_t o = 0;
    CoefUse mine;  // the table's generation, then noted for the caller's batch too
    if (!p->missing.empty()) {
        CoefUse* outer = coef_use_swap(&mine);
        const int rc = decode_coef(dev, *p, data_only, &o);
        coef_use_swap(outer);
        MXEC_TRY(rc);
        coef_note_use(mine.lo, mine.seq);
    }
    {
        std::lock_guard<std::mutex> g(dev.coef_mu);
        // Only remember the offset while its generation is live (a recycle
        // may have come between the upload and here).
        const uint64_t gen = mine.any() ? mine.lo : dev.coef_gen;
        if (gen + 1 >= dev.coef_gen) dev.patterns.emplace(key, Device::PatternVal{p, o, gen, mine.seq});
    }
    *plan = p;
    *off = o;
    return MXEC_OK;
}

int decode_step(Device& dev, Slot& slot, hipStream_t s, std::vector<DecodeItem> items, bool data_only,
                std::vector<std::shared_ptr<const DecodePlan>>& plans, uint64_t off, uint64_t pw, DescArena* arena,
                uint32_t max_blocks) {
    plans.assign(items.size(), nullptr);
    DecodeTables tables;
    auto collect = [&]() -> int {
        for (size_t t = 0; t < items.size(); ++t) {
            DecodeItem& it = items[t];
            if (it.S > off) MXEC_TRY(decode_plan(dev, it.k, it.m, it.present, data_only, &plans[t], &it.coef_off));
            it.plan = plans[t].get();
        }
        return MXEC_OK;
    };
    // The tables are rebuilt on every run: a re-run after a recycle of the
    // coefficient arena carries the fresh offsets.
    auto launch = [&]() -> int {
        const auto groups = tables.build(items, off, pw);
        return groups.empty() ? MXEC_OK : run_rs_mixed(dev, slot, s, groups, arena, max_blocks);
    };
    return with_stable_coef(dev, s, collect, launch);
}

namespace {
// A locate launch's (k, m) table into out (locate_table_bytes(m) bytes).
int locate_table(int k, int m, uint8_t* out) {
    auto mat = rs_matrix(k, m);
    if (!mat) return set_error(MXEC_E_SINGULAR_MATRIX, "encoding matrix construction failed");
    const int rc = locate_build_table(&mat->v[size_t(k) * size_t(k)], k, m, out);
    if (rc) return set_error(rc, "locate: the parity rows do not tell the data shards apart");
    return MXEC_OK;
}
}  // namespace

int run_rs(Device& dev, Slot& slot, hipStream_t s, uint64_t shard_size, int k, int r,
           const std::vector<RsObject>& objs, DescArena* arena, bool tune, uint32_t max_blocks) {
    if (objs.empty() || r == 0) return MXEC_OK;
    const size_t n = objs.size();
    if (affinity_on(dev)) {
        std::vector<const void*> ps;
        for (const RsObject& ob : objs) {
            for (int j = 0; j < k; ++j) ps.push_back(ob.in[j]);
            for (int i = 0; i < r; ++i) ps.push_back(ob.out[i]);
            for (int i = 0; i < r && ob.seed; ++i) ps.push_back(ob.seed[i]);
        }
        MXEC_TRY(affinity_check(dev, &slot, s, "run_rs", arena, ps.data(), ps.size()));
    }
    // Aligned launches handle length boundaries inside the fast kernel; an
    // unaligned pointer sends every tile to the byte-exact edge kernel.
    bool aligned = true;
    for (size_t o = 0; o < n && aligned; ++o) aligned = rs_aligned(objs[o], k, r);
    const RsPass pass = rs_pass_of(objs[0]);
    const bool locate = pass == kRsLocate;  // r = m in 2..8: one row block
    const bool verify = pass != kRsStore;
    RsTable t = RsTable::uniform(n, k, r, shard_size, rs_tile_bytes(rs_default_variant(uint32_t(r))), aligned, pass);
    // A seeded store (every object or none, RsObject::seed): the encode's
    // launch from seed rows.  Its k is a window's, so the tuner neither
    // times it nor lends it a grid.
    t.seeded = objs[0].seed != nullptr;
    for (const RsObject& ob : objs)
        if ((ob.seed != nullptr) != t.seeded || (t.seeded && verify))
            return set_error(MXEC_E_INVALID_ARG, "a seed is for every object of a store launch or none");
    if (t.seeded) tune = false;
    if (locate) {
        if (r < 2 || r > 8) return set_error(MXEC_E_INVALID_ARG, "locate needs 2..8 parity rows");
        t.locate_k(k);  // one table, every object's offset zero
    }
    DescWriter w(slot, arena);
    t.lay(w, true);
    char* hb = w.data();
    if (locate) MXEC_TRY(rs_locate_fill(hb, &t, 1, locate_table));
    for (const RsObject& ob : objs) t.put(hb, ob, k, r, shard_size);
    char* db = nullptr;
    MXEC_TRY(w.commit(s, &db));
    RsArgs a = t.args(db);
    a.coef = static_cast<const uint32_t*>(dev.coef.p);
    a.shard_size = shard_size;
    a.k = uint32_t(k);
    a.max_blocks = max_blocks ? max_blocks : dev.kn ? dev.kn->test_rs_grid : 0u;
    if (max_blocks || verify) tune = false;  // the tuner times encodes and decodes only
    // Large aligned single-launch batches take the grid tuner's pick.
    GridTuner::Trial trial;
    const double gb = double(n) * double(k + r) * double(shard_size) / 1e9;
    if (aligned && r <= 4 && tune) MXEC_TRY(rs_grid_pick(dev, k, r, shard_size, gb, &a.blocks_per_cu, &trial));
    // A verify walks the same tiles as the encode of its shape: the grid the
    // tuner settled on for that, if it has (0: the default).
    if (verify && aligned && r <= 4 && !max_blocks) a.blocks_per_cu = uint32_t(rs_grid_in_use(dev, k, r, shard_size));
    hipError_t e = trial.a ? hipEventRecord(trial.a, s) : hipSuccess;
    for (int row0 = 0; row0 < r && e == hipSuccess; row0 += 8) {
        a.row0 = uint32_t(row0);
        a.r = uint32_t(std::min(8, r - row0));
        e = launch_rs_apply(a, dev.n_cus, s);
    }
    if (trial.a && e == hipSuccess) e = hipEventRecord(trial.b, s);
    if (trial.a) {
        if (e == hipSuccess) {
            rs_grid_record(dev, k, r, shard_size, trial);
        } else {  // the trial's events are ours to free on a failed launch
            (void)hipEventDestroy(trial.a);
            (void)hipEventDestroy(trial.b);
        }
    }
    MXEC_HIP(e);
    return w.finish(s);
}

namespace {
// Tuning pays only where a launch is long enough for the grid to matter
// and an event pair costs nothing next to it.
constexpr double kTuneMinGB = 1.0;

bool tuning_on(const Device& dev) {
    if (dev.kn && (!dev.kn->rs_tune || dev.kn->test_rs_grid)) return false;
#ifdef MXEC_LAB
    if (getenv("MXEC_RS_BPC")) return false;  // a lab override fixes the grid
#endif
    return true;
}

// The candidate with the best time per GB (ties: the lower index).
int tuner_best(const GridTuner::State& st) {
    int b = 0;
    for (int c = 1; c < GridTuner::kCands; ++c)
        if (st.best_ms_per_gb[c] < st.best_ms_per_gb[b]) b = c;
    return b;
}

// Reads every finished trial of a shape into its best times; decides once
// every candidate has two samples (launches 2-7 of the shape cycle through
// the three grids).
void tuner_poll(GridTuner::State& st) {
    for (size_t i = 0; i < st.pending.size();) {
        GridTuner::Trial& t = st.pending[i];
        if (hipEventQuery(t.b) != hipSuccess) {
            (void)hipGetLastError();
            ++i;
            continue;
        }
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess && t.gb > 0) {
            st.best_ms_per_gb[t.cand] = std::min(st.best_ms_per_gb[t.cand], double(ms) / t.gb);
            ++st.samples[t.cand];
        }
        (void)hipGetLastError();
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
        st.pending.erase(st.pending.begin() + long(i));
    }
    bool all = true;
    for (int c = 0; c < GridTuner::kCands; ++c) all = all && st.samples[c] >= 2;
    if (st.decided < 0 && all) st.decided = tuner_best(st);
}
}  // namespace

int rs_grid_pick(Device& dev, int k, int r, uint64_t shard_size, double gb, uint32_t* bpc,
                 GridTuner::Trial* trial) {
    *bpc = 0;
    if (!tuning_on(dev) || gb < kTuneMinGB) return MXEC_OK;
    std::lock_guard<std::mutex> g(dev.tuner.mu);
    const auto key = std::make_tuple(k, r, shard_size);
    // A server sees a handful of shapes; past 256 new ones keep the default.
    if (dev.tuner.states.size() >= 256 && !dev.tuner.states.count(key)) return MXEC_OK;
    GridTuner::State& st = dev.tuner.states[key];
    if (!st.cands[0]) {
        st.cands[0] = rs_default_variant(uint32_t(r)).blocks_per_cu;
        st.cands[1] = st.cands[0] / 2;  // r <= 2: 1024 / 512 / 256; r = 3, 4: 512 / 256 / 128
        st.cands[2] = st.cands[0] / 4;
    }
    tuner_poll(st);
    if (st.decided >= 0) {
        *bpc = uint32_t(st.cands[st.decided]);
        return MXEC_OK;
    }
    constexpr int kTrials = 2 * GridTuner::kCands;
    if (st.launches > kTrials) {
        // Launches 2-7 were the trials (two per grid) and some still run (a
        // caller that queues far ahead): the default grid until their events
        // complete -- never a host wait inside an enqueue-only call.
        if (st.pending.empty()) st.decided = tuner_best(st);
        *bpc = uint32_t(st.cands[st.decided >= 0 ? st.decided : 0]);
        return MXEC_OK;
    }
    const int l = st.launches++;
    if (l == 0) return MXEC_OK;  // first launch of a shape: cold, untimed
    trial->cand = (l - 1) % GridTuner::kCands;
    trial->gb = gb;
    MXEC_HIP(hipEventCreate(&trial->a));
    if (hipEventCreate(&trial->b) != hipSuccess) {
        (void)hipEventDestroy(trial->a);
        trial->a = nullptr;
        return set_error(MXEC_E_DEVICE, "hipEventCreate failed");
    }
    *bpc = uint32_t(st.cands[trial->cand]);
    return MXEC_OK;
}

void rs_grid_record(Device& dev, int k, int r, uint64_t shard_size, const GridTuner::Trial& trial) {
    std::lock_guard<std::mutex> g(dev.tuner.mu);
    dev.tuner.states[std::make_tuple(k, r, shard_size)].pending.push_back(trial);
}

int rs_grid_in_use(Device& dev, int k, int r, uint64_t shard_size) {
    const int def = rs_default_variant(uint32_t(r)).blocks_per_cu;
#ifdef MXEC_LAB
    if (const char* e = getenv("MXEC_RS_BPC")) {
        const int b = atoi(e);
        if (b > 0 && b <= 4096) return b;
    }
#endif
    std::lock_guard<std::mutex> g(dev.tuner.mu);
    auto it = dev.tuner.states.find(std::make_tuple(k, r, shard_size));
    if (it == dev.tuner.states.end()) return def;
    tuner_poll(it->second);
    return it->second.decided >= 0 ? it->second.cands[it->second.decided] : 0;
}

void rs_grid_release(Device& dev) {
    std::lock_guard<std::mutex> g(dev.tuner.mu);
    for (auto& kv : dev.tuner.states)
        for (auto& t : kv.second.pending) {
            (void)hipEventDestroy(t.a);
            (void)hipEventDestroy(t.b);
        }
    dev.tuner.states.clear();
}

int run_rs_mixed(Device& dev, Slot& slot, hipStream_t s, const std::map<int, std::vector<RsMixedObject>>& groups,
                 DescArena* arena, uint32_t cap) {
    // Verify and locate hold for every object of a call or none (RsObject).
    RsPass pass = kRsStore;
    for (const auto& g : groups)
        if (!g.second.empty()) {
            pass = rs_pass_of(g.second[0].o);
            break;
        }
    const bool locate = pass == kRsLocate;
    // Which objects take grouped launches, which one run_rs per (k, shard
    // size), and whether the grouped launches fuse into one multi-r launch
    // (rs_plan.hpp; MXEC_RS_MULTI=0 keeps one launch per r).
    const uint64_t m_tile = rs_tile_bytes(rs_group_variant(kMultiR));
    const RsMixedPlan plan = rs_plan_mixed(
        groups, [](int r) { return rs_tile_bytes(rs_group_variant(uint32_t(r))); }, m_tile,
        !dev.kn || dev.kn->rs_multi, pass != kRsStore);
    for (const RsMixedPlan::Rest& u : plan.rest)
        MXEC_TRY(run_rs(dev, slot, s, u.shard_size, u.k, u.r, u.objs, arena, true, cap));
    if (plan.grouped.empty()) return MXEC_OK;
    if (affinity_on(dev)) {
        std::vector<const void*> ps;
        for (const RsMixedPlan::Group& g : plan.grouped)
            for (const RsMixedObject& ob : g.objs) {
                for (int j = 0; j < ob.k; ++j) ps.push_back(ob.o.in[j]);
                for (int i = 0; i < g.r; ++i) ps.push_back(ob.o.out[i]);
            }
        MXEC_TRY(affinity_check(dev, &slot, s, "run_rs_mixed", arena, ps.data(), ps.size()));
    }
    // One table per launch: the multi-r launch's over every group, or one
    // per grouped launch.
    std::vector<RsTable> ts;
    if (plan.multi) ts.push_back(RsTable::grouped(plan.m_obj, plan.m_k, plan.m_tiles, kMultiR, m_tile, pass, true));
    for (const RsMixedPlan::Group& g : plan.grouped) {
        if (plan.multi) break;  // never a verify or a locate
        ts.push_back(RsTable::grouped(g.objs.size(), g.sum_k, g.n_tiles, uint32_t(g.r), g.tile, pass));
        if (!locate) continue;
        if (g.r < 2 || g.r > 8) return set_error(MXEC_E_INVALID_ARG, "locate needs 2..8 parity rows");
        for (const RsMixedObject& ob : g.objs) ts.back().locate_k(ob.k);
    }
    // Every grouped launch's tables in one upload: one host-to-device copy
    // ahead of the launches instead of one between each pair of them (a
    // copy in the stream costs ~25-50 us of idle GPU at that point).
    DescWriter w(slot, arena);
    for (RsTable& t : ts) t.lay(w, false);
    const size_t o_lf = locate ? w.add(kLocateFieldBytes) : 0;
    for (RsTable& t : ts) t.o_lf = o_lf;
    char* hb = w.data();
    if (locate) MXEC_TRY(rs_locate_fill(hb, ts.data(), ts.size(), locate_table));
    for (size_t i = 0; i < plan.grouped.size(); ++i)
        for (const RsMixedObject& ob : plan.grouped[i].objs)
            ts[plan.multi ? 0 : i].put(hb, ob.o, ob.k, plan.grouped[i].r, ob.shard_size);
    char* db = nullptr;
    MXEC_TRY(w.commit(s, &db));
    for (const RsTable& t : ts) {
        RsArgs a = t.args(db);
        a.coef = static_cast<const uint32_t*>(dev.coef.p);
        a.max_blocks = cap ? cap : dev.kn ? dev.kn->test_rs_grid : 0u;
        MXEC_HIP(launch_rs_apply(a, dev.n_cus, s));
    }
    return w.finish(s);
}

int run_sha(Device& dev, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
            const std::vector<uint64_t>& lens, uint8_t* digests_dev, const uint8_t* expected_dev,
            uint8_t* ok_dev, const std::vector<uint64_t>* exp_idx, DescArena* arena, int form,
            const uint32_t** tmo_dev) {
    const size_t n = ptrs.size();
    if (tmo_dev) *tmo_dev = nullptr;
    if (!n) return MXEC_OK;
    if (affinity_on(dev)) {
        std::vector<const void*> ps(ptrs.begin(), ptrs.end());
        ps.push_back(digests_dev);
        ps.push_back(ok_dev);
        MXEC_TRY(affinity_check(dev, &slot, s, "run_sha", arena, ps.data(), ps.size()));
    }
    // The stream form: more 64-message groups than SIMDs, every message
    // 16-byte aligned, a caller that checks the timeout word, ring tables.
    // MXEC_SHA_FORM=stream forces it whenever it is allowed (tests); one,
    // split and lagpair pin the other forms the auto choice takes.
    const uint64_t groups = (n + 63) / 64, simds = uint64_t(dev.n_cus) * 4;
    const int env_form = dev.kn ? dev.kn->sha_form : 0;
    uint64_t longest = 0;
    for (uint64_t l : lens) longest = std::max(longest, l);
    const uint64_t seg_max = sha_stream_seg_max(longest, kShaSegBlocks);
    // The stream kernel's 32-bit item counter must not wrap (sha_plan.hpp).
    const bool items_fit = sha_stream_items_fit(n, seg_max, simds);
    bool stream = false;
    if (!items_fit) {
        // many messages plus one very long one: the split / one-wave forms
    } else if (tmo_dev && !arena && (form == kShaAuto || form == kShaStream) && n < (uint64_t(1) << 31)) {
        bool aligned = true;
        for (const uint8_t* p : ptrs) aligned = aligned && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
        stream = aligned && (sha_stream_size(groups, simds) || form == kShaStream || env_form == kShaStream);
    } else if (tmo_dev && !arena && env_form == kShaStream && n < (uint64_t(1) << 31)) {
        bool aligned = true;
        for (const uint8_t* p : ptrs) aligned = aligned && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
        stream = aligned;
    }
    DescWriter w(slot, arena);
    const size_t o_p = w.add(sizeof(void*) * n);
    const size_t o_l = w.add(8 * n);
    const size_t o_e = exp_idx ? w.add(8 * n) : 0;
    // Zeroed by the upload: [0] item counter, [1] timeout code, [4 + g] progress.
    const size_t o_w = stream ? w.add(4 * (4 + groups)) : 0;
    char* hb = w.data();
    std::memcpy(hb + o_p, ptrs.data(), sizeof(void*) * n);
    std::memcpy(hb + o_l, lens.data(), 8 * n);
    if (exp_idx) std::memcpy(hb + o_e, exp_idx->data(), 8 * n);
    char* db = nullptr;
    MXEC_TRY(w.commit(s, &db));
    ShaArgs a{};
    a.ptrs = reinterpret_cast<const uint8_t* const*>(db + o_p);
    a.lens = reinterpret_cast<const uint64_t*>(db + o_l);
    a.digests = digests_dev;
    a.expected = expected_dev;
    a.exp_idx = exp_idx ? reinterpret_cast<const uint64_t*>(db + o_e) : nullptr;
    a.ok = ok_dev;
    a.n = uint32_t(n);
    a.n_cus = uint32_t(dev.n_cus);
    a.force = form == kShaStream && !stream ? kShaAuto : form;
    if (a.force == kShaAuto && (env_form == kShaOneWave || env_form == kShaSplit || env_form == kShaLagPair))
        a.force = env_form;
    if (stream) {
        void* st = nullptr;
        MXEC_TRY(w.scratch(32 * n, &st));
        a.force = kShaStream;
        a.work = reinterpret_cast<uint32_t*>(db + o_w);
        a.state = static_cast<uint32_t*>(st);
        // One persistent wave per SIMD: 1.54 TB/s hashed from 65 536 to
        // 98 304 x 1 MiB, the chip's INT32 issue ceiling for this mix; two
        // per SIMD measured slower (131 072 x 1 MiB: 132.5 vs 92.8 ms for the
        // one-wave form; profiles/r2_sha_stream_lab.txt).
        a.waves = uint32_t(simds);
        // Four waves per workgroup: the dispatcher spreads a workgroup's
        // waves over the CU's four SIMDs, while one-wave workgroups after an
        // HBM-heavy kernel landed two to a SIMD on ~100 SIMDs and none on as
        // many, and the segment chains through the doubled SIMDs ran the
        // launch at half speed (81 920 x 1 MiB after an 8 GiB write kernel:
        // 110 ms vs 56; tools/sha_stream_lab place / repeat,
        // profiles/r2_sha_stream_placement.txt).
        a.wg_waves = simds % 4 == 0 ? 4 : 1;
        a.seg_max = uint32_t(seg_max);
        *tmo_dev = a.work + 1;
    }
    MXEC_HIP(launch_sha256(a, s));
    return w.finish(s);
}

int run_sha_pieces(Device& dev, Slot& slot, hipStream_t s, const std::vector<const uint8_t*>& ptrs,
                   const std::vector<uint64_t>& lens, const std::vector<uint32_t>& slots,
                   const std::vector<uint64_t>& totals, uint32_t* state_dev, bool resume, uint8_t* digests_dev,
                   DescArena* arena, const uint8_t* expected_dev, uint8_t* ok_dev) {
    const size_t n = ptrs.size();
    if (!n) return MXEC_OK;
    if (lens.size() != n || slots.size() != n || totals.size() != n || !state_dev ||
        n > uint64_t(kShaLagMsgs) * uint64_t(dev.n_cus ? dev.n_cus : 256))
        return set_error(MXEC_E_INVALID_ARG, "sha pieces: table sizes or message count");
    for (size_t i = 0; i < n; ++i)
        if (totals[i] == kShaNotFinal ? lens[i] % 64 != 0 : totals[i] < lens[i])
            return set_error(MXEC_E_INVALID_ARG, "sha pieces: a mid-message piece must be whole 64-byte blocks");
    if (affinity_on(dev)) {
        std::vector<const void*> ps(ptrs.begin(), ptrs.end());
        ps.push_back(digests_dev);
        ps.push_back(state_dev);
        MXEC_TRY(affinity_check(dev, &slot, s, "run_sha_pieces", arena, ps.data(), ps.size()));
    }
    DescWriter w(slot, arena);
    const size_t o_p = w.add(sizeof(void*) * n);
    const size_t o_l = w.add(8 * n);
    const size_t o_t = w.add(8 * n);
    const size_t o_s = w.add(4 * n);
    char* hb = w.data();
    std::memcpy(hb + o_p, ptrs.data(), sizeof(void*) * n);
    std::memcpy(hb + o_l, lens.data(), 8 * n);
    std::memcpy(hb + o_t, totals.data(), 8 * n);
    std::memcpy(hb + o_s, slots.data(), 4 * n);
    char* db = nullptr;
    MXEC_TRY(w.commit(s, &db));
    ShaArgs a{};
    a.ptrs = reinterpret_cast<const uint8_t* const*>(db + o_p);
    a.lens = reinterpret_cast<const uint64_t*>(db + o_l);
    a.digests = digests_dev;
    a.expected = expected_dev;
    a.ok = ok_dev;
    a.n = uint32_t(n);
    a.n_cus = uint32_t(dev.n_cus);
    a.force = kShaLagPair;
    a.piece.state = state_dev;
    a.piece.slot = reinterpret_cast<const uint32_t*>(db + o_s);
    a.piece.total = reinterpret_cast<const uint64_t*>(db + o_t);
    a.piece.resume = resume ? 1u : 0u;
    MXEC_HIP(launch_sha256(a, s));
    return w.finish(s);
}

}  // namespace mxec
