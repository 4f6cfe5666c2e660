// reconstruct.cpp — the reconstructs of include/maxio_ec.h over one object's
// host shards (mxec_reconstruct) and over device memory
// (mxec_reconstruct_strided_device, mxec_reconstruct_batch_device); the host
// batch is pipeline_get.cpp.  try_reconstruct_data_chunk's rules
// (chunk_reader.rs:157-226) per object: a digest mismatch is an erasure, the
// missing shards come from the first k present ones, an object short of k
// shards fails.  An object is a DecodeItem (its shards on the device, len and
// present on the host), every decode ops.cpp's decode_step.  No exception
// crosses the ABI.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>

#include "ops.hpp"

using namespace mxec;

namespace {

// len[i] = shard_len[i] clamped to the shard size S; S without a table.
template <class T>
void clamp_lens(const T* shard_len, uint64_t S, int n, uint64_t* len) {
    for (int i = 0; i < n; ++i) len[i] = shard_len ? std::min<uint64_t>(shard_len[i], S) : S;
}

// The present shards of a batch as messages to hash; idx: each one's global
// shard index (the objects' k + m one after another).
struct Present {
    std::vector<const uint8_t*> ptrs;
    std::vector<uint64_t> lens, idx;
};
Present present_shards(const std::vector<DecodeItem>& bo) {
    Present p;
    uint64_t g = 0;
    for (const DecodeItem& b : bo)
        for (int i = 0; i < b.k + b.m; ++i, ++g)
            if (b.present[i]) {
                p.ptrs.push_back(b.shard(i));
                p.lens.push_back(b.len[i]);
                p.idx.push_back(g);
            }
    return p;
}

// Rebuilds objects `which` of a batch from their present masks as they stand
// (chunk_reader.rs:190-211 per object): one decode plan per object, one launch
// per number of shards to rebuild, shared by objects of every (k, m) and
// shard size (decode_step).  Rebuilt shards become present; an object short
// of k shards gets MXEC_E_TOO_FEW_SHARDS_PRESENT in st.
int rebuild_batch(Device& d, Slot& slot, hipStream_t s, bool data_only, const std::vector<DecodeItem>& all,
                  const std::vector<uint64_t>& which, std::vector<int32_t>& st) {
    std::vector<DecodeItem> items;
    items.reserve(which.size());
    for (uint64_t o : which) items.push_back(all[o]);
    std::vector<std::shared_ptr<const DecodePlan>> plans;
    MXEC_TRY(decode_step(d, slot, s, std::move(items), data_only, plans));
    for (size_t t = 0; t < which.size(); ++t) {
        st[which[t]] = plans[t] ? MXEC_OK : MXEC_E_TOO_FEW_SHARDS_PRESENT;
        if (plans[t])
            for (int e : plans[t]->missing) all[which[t]].present[e] = 1;
    }
    return MXEC_OK;
}

// Hashes the device shards of `p` in one launch on `s` and compares on the
// device (the verify kernel compares message t against expected_dev[idx[t]]);
// the flags and the stream form's timeout word are read back, and a mismatch
// is an erasure: present[idx[t]] = 0 (chunk_reader.rs:176-196).
int verify_digests_device(Device& d, Slot& slot, hipStream_t s, const Present& p, const uint8_t* expected_dev,
                          uint8_t* present) {
    MXEC_TRY(slot.digests.grow(p.ptrs.size()));
    auto* ok = static_cast<uint8_t*>(slot.digests.p);
    const uint32_t* tmo = nullptr;
    MXEC_TRY(run_sha(d, slot, s, p.ptrs, p.lens, nullptr, expected_dev, ok, &p.idx, nullptr, 0, &tmo));
    const size_t fo = (p.ptrs.size() + 15) & ~size_t(15);
    MXEC_TRY(slot.hdig.grow(fo + 16));
    auto* hflag = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(slot.hdig.p) + fo);
    *hflag = 0;
    MXEC_HIP(hipMemcpyAsync(slot.hdig.p, ok, p.ptrs.size(), hipMemcpyDeviceToHost, s));
    if (tmo) MXEC_HIP(hipMemcpyAsync(hflag, tmo, 4, hipMemcpyDeviceToHost, s));
    MXEC_TRY(slot_wait(slot, s));
    if (*hflag != 0)
        return set_error(MXEC_E_DEVICE, "SHA-256 stream kernel: a wave timed out waiting for its predecessor segment");
    const auto* okh = static_cast<const uint8_t*>(slot.hdig.p);
    for (size_t t = 0; t < p.idx.size(); ++t)
        if (!okh[t]) present[p.idx[t]] = 0;
    return MXEC_OK;
}

// A small batch of one (k, m): hashed by the device's combiner together with
// every concurrent caller's verification (combiner.cpp), once the work queued
// on `stream` has produced the shards; digests compared on the host.  The
// combined launch waits for that work on the device (an event recorded here),
// not the host.
//
// Speculative rebuild: the decode from the present mask as given is queued
// right behind that event, so it runs beside the hash instead of after it
// (the hash is a VALU-bound chain, the decode an HBM stream).  It reads only
// present shards and writes only missing ones, which the hash does not read.
// Objects whose digests all match keep it -- exactly what verify-then-rebuild
// produces; an object with a mismatch is rebuilt again from its original mask
// minus the mismatched shards, over the same output shards, in stream order
// (chunk_reader.rs:176-211 semantics).  An object that ends up short of k
// shards may have its missing shards overwritten by the speculative decode.
int verify_combined_speculating(Device& d, Slot& slot, hipStream_t s, bool data_only,
                                const std::vector<DecodeItem>& bo, const Present& p, const uint8_t* expected_dev,
                                uint8_t* present, std::vector<int32_t>& st) {
    const uint64_t n_obj = bo.size();
    const int total = bo[0].k + bo[0].m;
    std::vector<uint64_t> all(static_cast<size_t>(n_obj));
    for (uint64_t o = 0; o < n_obj; ++o) all[o] = o;
    const size_t ne = size_t(n_obj) * size_t(total) * 32;
    MXEC_TRY(slot.hdig.grow(ne));
    MXEC_HIP(hipMemcpyAsync(slot.hdig.p, expected_dev, ne, hipMemcpyDeviceToHost, s));
    if (!slot.ready_ev) MXEC_HIP(hipEventCreateWithFlags(&slot.ready_ev, hipEventDisableTiming));
    MXEC_HIP(hipEventRecord(slot.ready_ev, s));
    const std::vector<uint8_t> orig(present, present + n_obj * uint64_t(total));
    // Queued by the combiner's leader right after the hash launch, so the
    // host work of the plans does not hold back the hash (or this caller's
    // arrival with it).
    const std::function<int()> spec = [&] { return rebuild_batch(d, slot, s, data_only, bo, all, st); };
    std::vector<uint8_t> dig(p.ptrs.size() * 32);
    if (int hrc = sha256_combined(d, slot, s, p.ptrs, p.lens, dig.data(), slot.ready_ev, &spec)) {
        // No verdict: the mask goes back as it came (the speculative rebuild
        // may already have marked shards present).
        const std::string msg = last_error();
        std::memcpy(present, orig.data(), orig.size());
        (void)slot_wait(slot, s);  // the speculative decode, if queued
        return set_error(hrc, msg);
    }
    MXEC_TRY(slot_wait(slot, s));  // the digest copy (long done), the speculative decode
    const auto* exph = static_cast<const uint8_t*>(slot.hdig.p);
    std::vector<uint64_t> redo;
    for (size_t t = 0; t < p.idx.size(); ++t) {
        if (std::memcmp(&dig[t * 32], exph + p.idx[t] * 32, 32) == 0) continue;
        const uint64_t o = p.idx[t] / uint64_t(total);
        if (redo.empty() || redo.back() != o) {
            redo.push_back(o);  // idx ascends: objects arrive in order
            std::memcpy(present + o * total, &orig[o * total], size_t(total));
        }
    }
    for (size_t t = 0; t < p.idx.size(); ++t)
        if (std::memcmp(&dig[t * 32], exph + p.idx[t] * 32, 32) != 0) present[p.idx[t]] = 0;
    return rebuild_batch(d, slot, s, data_only, bo, redo, st);
}

// How a device reconstruct verifies its present shards against
// expected_sha_dev (tests/test_contract_gpu.py pins the difference).
enum class Verify {
    kOnDevice,      // always its own launch on `stream`, compared on the device, before the rebuild
    kCombineSmall,  // a batch sha_combines() takes: the combiner, the rebuild speculatively beside it
};

// The device reconstructs once their objects are listed (present: every
// object's flags, one object after another; s: NULL = the HIP null stream):
// verify if digests are given, rebuild, report.
int reconstruct_device(Device& d, Slot& slot, hipStream_t s, const std::vector<DecodeItem>& bo, uint8_t* present,
                       const uint8_t* expected_dev, uint32_t flags, Verify how, int32_t* status_out) {
    const bool data_only = (flags & MXEC_F_DATA_ONLY) != 0;
    std::vector<int32_t> st(bo.size(), MXEC_OK);
    const Present p = expected_dev ? present_shards(bo) : Present{};
    if (!p.ptrs.empty() && how == Verify::kCombineSmall && sha_combines(d, p.ptrs.size())) {
        MXEC_TRY(verify_combined_speculating(d, slot, s, data_only, bo, p, expected_dev, present, st));
    } else {
        // A batch that fills the chip: its own launch on s, n flags read back.
        if (!p.ptrs.empty()) MXEC_TRY(verify_digests_device(d, slot, s, p, expected_dev, present));
        std::vector<uint64_t> all(bo.size());
        for (size_t o = 0; o < bo.size(); ++o) all[o] = o;
        MXEC_TRY(rebuild_batch(d, slot, s, data_only, bo, all, st));
    }
    return reconstruct_status(bo.data(), bo.size(), present, st, status_out);
}

}  // namespace

extern "C" {

int mxec_reconstruct(mxec_ctx* ctx, int k, int m, size_t shard_size, uint8_t* const* shards, const size_t* shard_len,
                     const uint8_t (*expected_sha256)[32], uint8_t* present_inout, uint32_t flags, int* n_present) {
    return guarded([&] {
        MXEC_TRY(reconstruct_shape(k, m, shard_size));
        if (!shards || !present_inout) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const int total = k + m;
        std::vector<uint64_t> len(static_cast<size_t>(total));
        clamp_lens(shard_len, shard_size, total, len.data());
        for (int i = 0; i < total; ++i)
            if (!shards[i]) return set_error(MXEC_E_INVALID_ARG, "null shard buffer");
        DevScope ds;
        MXEC_TRY(ds.open(ctx, -1));
        Slot& slot = *ds.slot;
        hipStream_t s = slot.stream;
        const uint64_t sa = round_up(shard_size, kSlotAlign);
        MXEC_TRY(slot.shards.ensure(sa * uint64_t(total) + uint64_t(total) * 64));
        auto* base = static_cast<uint8_t*>(slot.shards.p);
        std::vector<uint8_t> present(present_inout, present_inout + total);
        // The one object: shard i in the slot's staging buffer at base + i * sa.
        const DecodeItem ob{k, m, shard_size, len.data(), present.data(), nullptr, base, sa};
        const Present p = present_shards({ob});
        std::vector<UploadSeg> up;
        for (size_t t = 0; t < p.idx.size(); ++t)
            if (p.lens[t]) up.push_back({sa * p.idx[t], shards[p.idx[t]], p.lens[t]});
        MXEC_TRY(upload_segments(slot, s, base, up, copy_waves_get(*ds.d)));
        if (expected_sha256 && !p.ptrs.empty()) {
            // chunk_reader.rs:176-196: hash every present shard; mismatch -> erasure.
            MXEC_TRY(slot_wait(slot, s));
            std::vector<uint8_t> dig(p.ptrs.size() * 32);
            MXEC_TRY(sha256_combined(*ds.d, slot, s, p.ptrs, p.lens, dig.data()));
            for (size_t t = 0; t < p.idx.size(); ++t)
                if (std::memcmp(&dig[t * 32], expected_sha256[p.idx[t]], 32) != 0) present[p.idx[t]] = 0;
        }
        const int np = total - int(std::count(present.begin(), present.end(), 0));
        if (n_present) *n_present = np;
        if (np < k) return set_error(MXEC_E_TOO_FEW_SHARDS_PRESENT, too_few_msg(np, k, total));
        // One item is one uniform group, which run_rs_mixed hands to run_rs
        // on the slot's ring with the grid tuner on (rs_plan_mixed).
        std::vector<std::shared_ptr<const DecodePlan>> plans;
        MXEC_TRY(decode_step(*ds.d, slot, s, {ob}, (flags & MXEC_F_DATA_ONLY) != 0, plans));
        if (!plans[0]) return set_error(MXEC_E_SINGULAR_MATRIX, "decode matrix inversion failed");
        const std::vector<int>& missing = plans[0]->missing;
        if (!missing.empty()) {
            std::vector<DownloadSeg> down;
            for (int e : missing)
                if (len[size_t(e)]) down.push_back({sa * uint64_t(e), shards[e], len[size_t(e)]});
            // missing is ascending, so are the offsets.
            MXEC_TRY(download_segments(slot, s, base, down, copy_waves_get(*ds.d)));
            for (int e : missing) present[size_t(e)] = 1;
        } else {
            // Nothing to rebuild: the uploads may still be reading the
            // caller's buffers (direct DMA from page-locked memory).
            MXEC_TRY(slot_wait(slot, s));
        }
        std::memcpy(present_inout, present.data(), size_t(total));
        return MXEC_OK;
    });
}

int mxec_reconstruct_strided_device(mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                                    uint64_t n_obj, uint8_t* shards, uint64_t obj_stride, uint64_t shard_stride,
                                    const uint64_t* shard_len, uint8_t* present, const uint8_t* expected_sha_dev,
                                    uint32_t flags, int32_t* status_out) {
    return guarded([&] {
        MXEC_TRY(reconstruct_shape(k, m, shard_size));
        if (n_obj == 0) return MXEC_OK;
        if (!shards || !present) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const int total = k + m;
        DevScope ds;
        MXEC_TRY(ds.open(ctx, dev));
        std::vector<uint64_t> len(static_cast<size_t>(total));
        clamp_lens(shard_len, shard_size, total, len.data());
        std::vector<DecodeItem> bo;
        bo.reserve(static_cast<size_t>(n_obj));
        for (uint64_t o = 0; o < n_obj; ++o)
            bo.push_back(DecodeItem{k, m, shard_size, len.data(), present + o * total, nullptr, shards + o * obj_stride,
                                    shard_stride});
        return reconstruct_device(*ds.d, *ds.slot, static_cast<hipStream_t>(stream), bo, present, expected_sha_dev,
                                  flags, Verify::kCombineSmall, status_out);
    });
}

int mxec_reconstruct_batch_device(mxec_ctx* ctx, int dev, void* stream, const mxec_object* objs, uint64_t n_obj,
                                  uint8_t* const* shards, const uint64_t* shard_len, uint8_t* present,
                                  const uint8_t* expected_sha_dev, uint32_t flags, int32_t* status_out) {
    return guarded([&] {
        if (n_obj == 0) return MXEC_OK;
        if (!objs || !shards || !present) return set_error(MXEC_E_INVALID_ARG, "null argument");
        uint64_t sum = 0;
        for (uint64_t o = 0; o < n_obj; ++o) {
            MXEC_TRY(reconstruct_shape(objs[o].k, objs[o].m, objs[o].shard_size));
            sum += uint64_t(objs[o].k + objs[o].m);
        }
        DevScope ds;
        MXEC_TRY(ds.open(ctx, dev));
        // Every shard pointer is needed: present ones are read, missing ones
        // are where the rebuilt bytes go (a NULL would fault the device).
        for (uint64_t g = 0; g < sum; ++g)
            if (!shards[g]) return set_error(MXEC_E_INVALID_ARG, "null shard pointer " + std::to_string(g));
        std::vector<uint64_t> len(static_cast<size_t>(sum));
        std::vector<DecodeItem> bo;
        bo.reserve(static_cast<size_t>(n_obj));
        uint64_t g0 = 0;
        for (uint64_t o = 0; o < n_obj; ++o) {
            const int total = objs[o].k + objs[o].m;
            clamp_lens(shard_len ? shard_len + g0 : nullptr, objs[o].shard_size, total, &len[g0]);
            bo.push_back(DecodeItem{objs[o].k, objs[o].m, objs[o].shard_size, &len[g0], present + g0, shards + g0,
                                    nullptr, 0});
            g0 += uint64_t(total);
        }
        return reconstruct_device(*ds.d, *ds.slot, static_cast<hipStream_t>(stream), bo, present, expected_sha_dev,
                                  flags, Verify::kOnDevice, status_out);
    });
}

}  // extern "C"
