// storage_scrub.cpp — one `{key}.ec` directory checked and repaired from its
// own shards: try_reconstruct_data_chunk (chunk_reader.rs:157-226) at the
// file level, mxec_scrub_object and mxec_locate_object (no reference: MaxIO
// has no scrubber).  All three load a ShardSet and decode it once.
#include <cstring>

#include "ops.hpp"
#include "scrub_plan.hpp"
#include "shard_set.hpp"

using namespace mxec;

extern "C" int mxec_try_reconstruct_data_chunk(mxec_ctx* ctx, const char* ec_dir, uint32_t target, uint8_t* out,
                                               uint64_t out_cap, uint64_t* out_len) {
    return guarded([&]() -> int {
        if (!ec_dir || !out_len) return set_error(MXEC_E_INVALID_ARG, "null argument");
        Manifest man;
        MXEC_TRY(read_manifest(ec_dir, man));
        if (target >= man.chunk_count) return set_error(MXEC_E_INVALID_INDEX, "target is not a data chunk");
        // Read every shard, verify it against the manifest digest, rebuild
        // the rest on the GPU.  Present shards are hashed over their on-disk
        // bytes, want(i) of them; a digest that is not the 64 lower-case
        // digits the reference's string compare can match (chunk_reader.rs:
        // 184-185) never matches, so that shard is an erasure too.
        ShardSet set;
        MXEC_TRY(set.open(man, ShardSet::kCheckAlways));
        std::vector<uint8_t> expected(size_t(set.total) * 32, 0);
        for (int i = 0; i < set.total; ++i)
            if (!(set.read(ec_dir, i) && manifest_digest32(man.chunks[size_t(i)].sha256, &expected[size_t(i) * 32])))
                set.blank(i, true);
        int np = 0;
        MXEC_TRY(set.decode(ctx, expected.data(), 0, &np));
        const size_t real = set.want(int(target));
        *out_len = real;
        if (real > out_cap || (real && !out)) return set_error(MXEC_E_INVALID_ARG, "output buffer too small");
        if (real) std::memcpy(out, set.ptrs[target], real);
        return MXEC_OK;
    });
}

// ---- scrub / heal ------------------------------------------------------------

namespace {

// The shard files, parity included, read and sized as try_reconstruct does;
// returns whether each is there at its size.  With `state` (total entries)
// all are read, a missing or wrong-sized one noted there and zero-filled
// where a heal rebuilds it; without, the first such ends it.
bool load(ShardSet& ob, const fs::path& dir, uint8_t* state) {
    bool whole = true;
    for (int i = 0; i < ob.total; ++i) {
        bool there = false;
        if (ob.read(dir, i, &there)) continue;
        whole = false;
        if (!state) break;
        state[i] = there ? MXEC_SHARD_BAD_SIZE : MXEC_SHARD_MISSING;
        ob.blank(i, true);
    }
    set_error(0, "");  // a missing file is a finding, not this call's error
    return whole;
}

// The heal: shards `bad` rebuilt from all the others as they are (the decode
// checks no digest) and hashed; only if each is what the manifest recorded
// (expected: total x 32 bytes, parsed: which of them parsed) are they written
// under their final names.  *wrote: files replaced, all of `bad` or none.
int rebuild_and_replace(mxec_ctx* ctx, const fs::path& dir, ShardSet& ob, const std::vector<int>& bad,
                        const std::vector<uint8_t>& expected, const std::vector<uint8_t>& parsed, size_t* wrote) {
    *wrote = 0;
    for (int i : bad) ob.blank(i, true);
    int np = 0;
    MXEC_TRY(ob.decode(ctx, nullptr, 0, &np));
    std::vector<const uint8_t*> hp;
    std::vector<size_t> hl;
    for (int i : bad) { hp.push_back(ob.ptrs[size_t(i)]); hl.push_back(ob.lens[size_t(i)]); }
    std::vector<uint8_t> dig(hp.size() * 32);
    MXEC_TRY(mxec_sha256_batch(ctx, hp.data(), hl.data(), hp.size(), reinterpret_cast<uint8_t(*)[32]>(dig.data())));
    for (size_t t = 0; t < bad.size(); ++t)
        if (!parsed[size_t(bad[t])] || std::memcmp(&dig[t * 32], &expected[size_t(bad[t]) * 32], 32) != 0)
            return MXEC_OK;  // more is wrong than the shards named
    for (size_t t = 0; t < bad.size(); ++t, ++*wrote)
        MXEC_TRY(replace_file(dir, chunk_name(uint32_t(bad[t])), hp[t], hl[t]));
    return MXEC_OK;
}

}  // namespace

extern "C" int mxec_scrub_object(mxec_ctx* ctx, const char* ec_dir, uint32_t flags, void* out) {
    return guarded([&]() -> int {
        if (!ec_dir || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (flags & ~(MXEC_SCRUB_PARITY | MXEC_SCRUB_DIGESTS | MXEC_SCRUB_HEAL))
            return set_error(MXEC_E_INVALID_ARG, "scrub: unknown flag");
        auto* rep = static_cast<mxec_scrub_report*>(out);
        std::memset(rep, 0, sizeof *rep);
        rep->parity_consistent = -1;
        rep->parity_first_bad = MXEC_VERIFY_OK;
        const fs::path dir(ec_dir);
        if (flags & MXEC_SCRUB_HEAL) flags |= MXEC_SCRUB_DIGESTS;
        Manifest man;
        MXEC_TRY(read_manifest(dir, man));
        ShardSet ob;  // an object without parity has nothing ReedSolomon::new would see
        MXEC_TRY(ob.open(man, ShardSet::kCheckParity));
        const int k = ob.k, m = ob.m, total = ob.total;
        if (total > int(sizeof rep->shard_state))
            return set_error(MXEC_E_INVALID_ARG, "scrub: more shards than the report holds (" + std::to_string(total) + ")");
        rep->k = uint32_t(k);
        rep->m = uint32_t(m);
        uint8_t* st = rep->shard_state;
        const bool whole = load(ob, dir, st);

        if ((flags & MXEC_SCRUB_PARITY) && m > 0 && whole) {
            std::vector<uint64_t> fb(static_cast<size_t>(m));
            int ok = 0;
            MXEC_TRY(mxec_verify(ctx, k, m, ob.shard, ob.ptrs.data(), ob.lens.data(), ob.ptrs.data() + k, fb.data(), &ok));
            rep->parity_consistent = ok;
            for (uint64_t v : fb) rep->parity_first_bad = std::min(rep->parity_first_bad, v);
        }

        std::vector<uint8_t> expected(size_t(total) * 32, 0);
        std::vector<uint8_t> parsed(static_cast<size_t>(total), 0);
        if (flags & MXEC_SCRUB_DIGESTS) {
            std::vector<const uint8_t*> hp;
            std::vector<size_t> hl;
            std::vector<int> hi;
            for (int i = 0; i < total; ++i) {
                parsed[size_t(i)] = manifest_digest32(man.chunks[size_t(i)].sha256, &expected[size_t(i) * 32]);
                if (st[i] != MXEC_SHARD_OK) continue;
                if (!parsed[size_t(i)]) {  // not what the GET's string compare can match (chunk_reader.rs:108-109)
                    st[i] = MXEC_SHARD_BAD_DIGEST;
                    continue;
                }
                hp.push_back(ob.ptrs[size_t(i)]);
                hl.push_back(ob.lens[size_t(i)]);
                hi.push_back(i);
            }
            std::vector<uint8_t> dig(hp.size() * 32);
            MXEC_TRY(mxec_sha256_batch(ctx, hp.data(), hl.data(), hp.size(), reinterpret_cast<uint8_t(*)[32]>(dig.data())));
            for (size_t t = 0; t < hi.size(); ++t)
                if (std::memcmp(&dig[t * 32], &expected[size_t(hi[t]) * 32], 32) != 0) st[hi[t]] = MXEC_SHARD_BAD_DIGEST;
        }

        rep->n_damaged = scrub_damaged(st, uint32_t(total));
        bool rebuilt_ok = false;
        if ((flags & MXEC_SCRUB_HEAL) && scrub_can_heal(rep->n_damaged, uint32_t(m))) {
            // Every damaged shard, data and parity, from the verified ones.
            std::vector<int> bad;
            for (int i = 0; i < total; ++i)
                if (st[i] != MXEC_SHARD_OK) bad.push_back(i);
            size_t wrote = 0;
            const int rc = rebuild_and_replace(ctx, dir, ob, bad, expected, parsed, &wrote);
            for (size_t t = 0; t < wrote; ++t) st[bad[t]] |= MXEC_SHARD_HEALED;
            rep->n_healed += uint32_t(wrote);
            MXEC_TRY(rc);
            rebuilt_ok = wrote == bad.size();
        }
        rep->verdict = scrub_verdict(rep->n_damaged, uint32_t(m), rep->parity_consistent, (flags & MXEC_SCRUB_HEAL) != 0,
                                     rebuilt_ok);
        return MXEC_OK;
    });
}

// The scrub's parity pass, naming the shard: no digest of any present shard.
// A heal rebuilds the one located shard and hashes that alone.
extern "C" int mxec_locate_object(mxec_ctx* ctx, const char* ec_dir, uint32_t flags, void* out) {
    return guarded([&]() -> int {
        if (!ec_dir || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        if (flags & ~MXEC_LOCATE_F_HEAL) return set_error(MXEC_E_INVALID_ARG, "locate: unknown flag");
        auto* rep = static_cast<mxec_locate_report*>(out);
        std::memset(rep, 0, sizeof *rep);
        rep->first_bad = MXEC_VERIFY_OK;
        const fs::path dir(ec_dir);
        Manifest man;
        MXEC_TRY(read_manifest(dir, man));
        ShardSet ob;
        MXEC_TRY(ob.open(man, ShardSet::kCheckParity));
        rep->k = uint32_t(ob.k);
        rep->m = uint32_t(ob.m);
        rep->outcome = MXEC_LOCATE_SKIPPED;
        if (ob.m < 2 || ob.m > 8) return MXEC_OK;
        // A shard that is missing or wrong-sized is the digest pass's to report.
        if (!load(ob, dir, nullptr)) return MXEC_OK;

        mxec_locate_result res;
        MXEC_TRY(mxec_locate(ctx, ob.k, ob.m, ob.shard, ob.ptrs.data(), ob.lens.data(), ob.ptrs.data() + ob.k, &res));
        rep->first_bad = res.first_bad;
        rep->n_bad = res.n_bad;
        rep->outcome = uint32_t(mxec_locate_outcome(&res, &rep->shard));
        if (!(flags & MXEC_LOCATE_F_HEAL) || rep->outcome != MXEC_LOCATE_ONE) return MXEC_OK;
        if (rep->shard >= uint32_t(ob.total)) return MXEC_OK;

        const std::vector<int> bad{int(rep->shard)};
        std::vector<uint8_t> expected(size_t(ob.total) * 32, 0), parsed(static_cast<size_t>(ob.total), 0);
        parsed[rep->shard] = manifest_digest32(man.chunks[rep->shard].sha256, &expected[size_t(rep->shard) * 32]);
        if (!parsed[rep->shard]) return MXEC_OK;  // nothing to check a rebuild against
        size_t wrote = 0;  // 0 when more is wrong than one shard: the scrub's heal
        MXEC_TRY(rebuild_and_replace(ctx, dir, ob, bad, expected, parsed, &wrote));
        rep->healed = wrote == 1;
        return MXEC_OK;
    });
}
