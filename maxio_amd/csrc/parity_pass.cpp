// parity_pass.cpp — the parity pass of include/maxio_ec.h: recompute every
// object's m parity rows from its k data shards, then store them (encode),
// compare them with the stored rows (verify) or classify the mismatches
// (locate); each from host pointers, a strided device batch or a mixed one.
// The strided encode also runs over a window of the data shards from a
// running parity (mxec_encode_update_strided_device).
#include <algorithm>

#include "../../include/maxio_ec.h"
#include "kernels.hpp"
#include "locate_plan.hpp"
#include "ops.hpp"

using namespace mxec;

static_assert(sizeof(mxec_locate_result) == 24 && sizeof(LocateRec) == sizeof(mxec_locate_result) &&
                  offsetof(LocateRec, n_bad) == offsetof(mxec_locate_result, n_bad) &&
                  offsetof(LocateRec, shard_min) == offsetof(mxec_locate_result, shard_min) &&
                  offsetof(LocateRec, shard_max) == offsetof(mxec_locate_result, shard_max),
              "the kernel's record is the header's");
static_assert(kLocateNoShard == MXEC_LOCATE_NO_SHARD, "one sentinel");

namespace {

// What a pass does with the recomputed rows and leaves at `result`: nothing
// (Store), a uint64 per parity row, the first differing offset (Compare), or
// a LocateRec per object (Locate).
enum class Policy { Store, Compare, Locate };
struct Pass { Policy p; void* result = nullptr; };  // device memory in the two bodies, the caller's in host_pass
struct Strided { const uint8_t* base; uint64_t obj_stride, shard_stride; };
// A window of a Store pass: data shards [first, first + count) of the k, the
// data base at shard `first`, folded into the rows at `seed` (null base: zeros).
struct Window { int first, count; Strided seed; };

// Bytes of result that `objs` objects with `rows` parity rows in all occupy.
uint64_t result_bytes(Policy p, uint64_t objs, uint64_t rows) {
    return p == Policy::Store ? 0 : p == Policy::Compare ? 8 * rows : sizeof(LocateRec) * objs;
}

// Locate: one parity row cannot tell shards apart, more than eight do not fit one row block.
int check_shape(Policy p, int k, int m, uint64_t shard_size) {
    MXEC_TRY(check_km(k, m));
    if (p == Policy::Locate && m < 2) return set_error(MXEC_E_INVALID_ARG, "locate needs at least two parity shards");
    if (p == Policy::Locate && m > 8) return set_error(MXEC_E_INVALID_ARG, "locate takes at most eight parity shards");
    if (shard_size == 0) return set_error(MXEC_E_EMPTY_SHARD, mxec_strerror(MXEC_E_EMPTY_SHARD));
    return MXEC_OK;
}

// A call's result entries as the kernels expect to find them: 0xFF (MXEC_VERIFY_OK) or fresh records.
int queue_init(const Pass& ps, uint64_t bytes, hipStream_t s) {
    if (ps.p == Policy::Compare) MXEC_HIP(hipMemsetAsync(ps.result, 0xFF, size_t(bytes), s));
    if (ps.p == Policy::Locate)
        MXEC_HIP(launch_locate_init(static_cast<LocateRec*>(ps.result), bytes / sizeof(LocateRec), s));
    return MXEC_OK;
}

// `parity` is written under Store and only read otherwise (rs_plan.hpp RsObject).
RsObject rs_object(const Pass& ps, const uint8_t* const* in, const uint8_t* const* parity, const uint64_t* len, int k,
                   uint32_t coef_off, uint64_t result_off) {
    RsObject ob{in, len, const_cast<uint8_t* const*>(parity), len + k, coef_off};
    uint8_t* r = static_cast<uint8_t*>(ps.result) + result_off;
    if (ps.p == Policy::Compare) ob.first_bad = reinterpret_cast<uint64_t*>(r);
    if (ps.p == Policy::Locate) ob.locate = r;
    return ob;
}

// The uniform body: n_obj objects of one (k, m, shard_size) and one table of
// k + m shard lengths.  digests_dev (Store only, or null): every shard's SHA-256.
// win (Store only, or null): the launch has the window's `count` inputs (len:
// count + m entries) and reads the (k, m) table from column `first` on -- its
// layout is [j][i][8], so a column range is contiguous.
int uniform_pass(Device& d, Slot& slot, hipStream_t s, const Pass& ps, int k, int m, uint64_t shard_size,
                 uint64_t n_obj, Strided data, Strided parity, const std::vector<uint64_t>& len, uint8_t* digests_dev,
                 const Window* win = nullptr) {
    const int kin = win ? win->count : k, total = kin + m;
    const bool seeded = win && win->seed.base;
    std::vector<const uint8_t*> sh(static_cast<size_t>(n_obj * total));  // per object: kin data, m parity
    std::vector<const uint8_t*> seeds(seeded ? static_cast<size_t>(n_obj * m) : 0);
    std::vector<RsObject> objs(static_cast<size_t>(n_obj));
    for (uint64_t o = 0; o < n_obj; ++o) {
        const uint8_t** p = &sh[o * total];
        for (int j = 0; j < kin; ++j) p[j] = data.base + o * data.obj_stride + j * data.shard_stride;
        for (int i = 0; i < m; ++i) p[kin + i] = parity.base + o * parity.obj_stride + i * parity.shard_stride;
        objs[o] = rs_object(ps, p, p + kin, len.data(), kin, 0, result_bytes(ps.p, o, o * m));
        for (int i = 0; i < m && seeded; ++i)
            seeds[o * m + i] = win->seed.base + o * win->seed.obj_stride + i * win->seed.shard_stride;
        if (seeded) objs[o].seed = &seeds[o * m];
    }
    uint32_t off = 0;
    MXEC_TRY(with_stable_coef(d, s, [&] { return encode_coef(d, k, m, &off); }, [&] {
        // Initialised inside the launch step: a pass queued again after a
        // table recycle (with_stable_coef) starts from clean entries, so
        // first_bad and n_bad are those of one pass.
        MXEC_TRY(queue_init(ps, result_bytes(ps.p, n_obj, n_obj * m), s));
        for (auto& ob : objs) ob.coef_off = off + (win ? uint32_t(win->first) * uint32_t(m) * 8u : 0u);
        return run_rs(d, slot, s, shard_size, kin, m, objs);
    }));
    std::vector<uint64_t> lens;
    for (uint64_t o = 0; o < n_obj && digests_dev; ++o) lens.insert(lens.end(), len.begin(), len.end());
    return digests_dev ? run_sha(d, slot, s, sh, lens, digests_dev, nullptr, nullptr) : MXEC_OK;
}

// Whether any seed row shares a byte with any row written.
bool rows_overlap(const Strided& a, const Strided& b, uint64_t n_obj, int m, uint64_t shard_size) {
    std::vector<std::pair<uintptr_t, int>> at;  // row starts: 0 = a, 1 = b
    for (uint64_t o = 0; o < n_obj; ++o)
        for (int i = 0; i < m; ++i) {
            at.emplace_back(reinterpret_cast<uintptr_t>(a.base) + o * a.obj_stride + i * a.shard_stride, 0);
            at.emplace_back(reinterpret_cast<uintptr_t>(b.base) + o * b.obj_stride + i * b.shard_stride, 1);
        }
    std::sort(at.begin(), at.end());
    uintptr_t end[2] = {0, 0};  // how far the rows of each side seen so far reach
    for (const auto& r : at) {
        if (r.first < end[1 - r.second]) return true;
        end[r.second] = std::max(end[r.second], r.first + uintptr_t(shard_size));
    }
    return false;
}

int strided_pass(const Pass& ps, mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                 uint64_t n_obj, Strided data, const uint64_t* data_len, Strided parity, uint8_t* digests_dev,
                 const Window* win = nullptr) {
    return guarded([&] {
        MXEC_TRY(check_shape(ps.p, k, m, shard_size));
        if (win && (win->first < 0 || win->count < 1 || win->first > k - win->count))
            return set_error(MXEC_E_INVALID_ARG, "window [" + std::to_string(win->first) + ", +" +
                                                     std::to_string(win->count) + ") is not within the " +
                                                     std::to_string(k) + " data shards");
        if (win && (!data.base || !parity.base)) return set_error(MXEC_E_INVALID_ARG, "null base pointer");
        if (win && win->seed.base && rows_overlap(win->seed, parity, n_obj, m, shard_size))
            return set_error(MXEC_E_INVALID_ARG, "parity_in and parity_out overlap");
        if (n_obj == 0) return MXEC_OK;
        if (!data.base || !parity.base) return set_error(MXEC_E_INVALID_ARG, "null base pointer");
        if (ps.p != Policy::Store && !ps.result) return set_error(MXEC_E_INVALID_ARG, "null result array");
        DevScope ds;
        MXEC_TRY(ds.open(ctx, dev));
        const int kin = win ? win->count : k;
        std::vector<uint64_t> len(static_cast<size_t>(kin + m), shard_size);
        for (int j = 0; j < kin && data_len; ++j) len[size_t(j)] = std::min<uint64_t>(data_len[j], shard_size);
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
        return uniform_pass(*ds.d, *ds.slot, s, ps, k, m, shard_size, n_obj, data, parity, len, digests_dev, win);
    });
}

// The mixed body: objects of their own (k, m, shard_size), pointers and
// lengths concatenated object-major, all checked before a device is touched.
// One launch per parity count m: objects of every k and shard size share it
// (run_rs_mixed; unaligned or m > 8: per (k, shard_size)).
int mixed_pass(const Pass& ps, mxec_ctx* ctx, int dev, void* stream, const mxec_object* objs, uint64_t n_obj,
               const uint8_t* const* data, const uint64_t* data_len, const uint8_t* const* parity,
               uint8_t* digests_dev) {
    return guarded([&] {
        if (n_obj == 0) return MXEC_OK;
        if (!objs || !data || !parity || (ps.p != Policy::Store && !ps.result))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        std::vector<uint64_t> dofs(static_cast<size_t>(n_obj)), pofs(dofs), len;  // len: per object k data, m parity
        std::vector<const uint8_t*> sh;                                           // the shards in that order
        uint64_t dsum = 0, psum = 0;
        for (uint64_t o = 0; o < n_obj; ++o) {
            const uint64_t S = objs[o].shard_size;
            MXEC_TRY(check_shape(ps.p, objs[o].k, objs[o].m, S));
            dofs[o] = dsum;
            pofs[o] = psum;
            for (int j = 0; j < objs[o].k; ++j, ++dsum) {
                len.push_back(data_len ? std::min<uint64_t>(data_len[dsum], S) : S);
                if (!data[dsum] && len.back())
                    return set_error(MXEC_E_INVALID_ARG, "null data pointer " + std::to_string(dsum));
            }
            for (int i = 0; i < objs[o].m; ++i, ++psum)
                if (!parity[psum]) return set_error(MXEC_E_INVALID_ARG, "null parity pointer " + std::to_string(psum));
            len.insert(len.end(), size_t(objs[o].m), S);
            sh.insert(sh.end(), data + dofs[o], data + dsum);
            sh.insert(sh.end(), parity + pofs[o], parity + psum);
        }
        DevScope ds;
        MXEC_TRY(ds.open(ctx, dev));
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
        std::map<int, std::vector<RsMixedObject>> groups;
        MXEC_TRY(with_stable_coef(*ds.d, s, [&]() -> int {
            groups.clear();
            std::map<std::pair<int, int>, uint32_t> offs;
            for (uint64_t o = 0; o < n_obj; ++o) {
                const int k = objs[o].k, m = objs[o].m;
                auto [it, fresh] = offs.try_emplace({k, m}, 0u);
                if (fresh) MXEC_TRY(encode_coef(*ds.d, k, m, &it->second));
                groups[m].push_back({k, objs[o].shard_size,
                                     rs_object(ps, data + dofs[o], parity + pofs[o], &len[dofs[o] + pofs[o]], k,
                                               it->second, result_bytes(ps.p, o, pofs[o]))});
            }
            return MXEC_OK;
        }, [&]() -> int {
            MXEC_TRY(queue_init(ps, result_bytes(ps.p, n_obj, psum), s));  // in the launch step, as in uniform_pass
            return run_rs_mixed(*ds.d, *ds.slot, s, groups);
        }));
        return digests_dev ? run_sha(*ds.d, *ds.slot, s, sh, len, digests_dev, nullptr, nullptr) : MXEC_OK;
    });
}

// One object from host pointers: the uniform body on a staged copy, shards
// round_up(shard_size, kSlotAlign) apart in slot.shards, the result behind
// them.  Store uploads the data and downloads the parity, the others upload
// both and download the result.  A chunk longer than shard_size is refused
// here, not clamped.
int host_pass(const Pass& ps, mxec_ctx* ctx, int k, int m, size_t shard_size, const uint8_t* const* data,
              const size_t* data_len, const uint8_t* const* parity, uint8_t (*sha256_out)[32]) {
    return guarded([&] {
        const bool store = ps.p == Policy::Store;
        MXEC_TRY(check_shape(ps.p, k, m, shard_size));
        if (!data || !parity || (!store && !ps.result)) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const uint64_t sa = round_up(shard_size, kSlotAlign), res_off = sa * uint64_t(k + m);
        std::vector<uint64_t> len(static_cast<size_t>(k + m), shard_size);
        std::vector<const uint8_t*> staged;
        std::vector<UploadSeg> up;
        std::vector<DownloadSeg> down;
        for (int i = 0; i < k + m; ++i) {
            const uint8_t* p = i < k ? data[i] : parity[i - k];
            uint64_t& l = len[size_t(i)];
            if (i < k && data_len) l = data_len[i];
            if (l > shard_size) return set_error(MXEC_E_INCORRECT_SHARD_SIZE, "data chunk longer than shard_size");
            if (l && !p) return set_error(MXEC_E_INVALID_ARG, "null shard " + std::to_string(i));
            if (l && (i < k || !store)) up.push_back({sa * uint64_t(i), p, l});
            if (i >= k && store) down.push_back({sa * uint64_t(i), const_cast<uint8_t*>(p), l});
        }
        if (!store) down.push_back({res_off, static_cast<uint8_t*>(ps.result), result_bytes(ps.p, 1, uint64_t(m))});
        DevScope ds;
        MXEC_TRY(ds.open(ctx, -1));
        Slot& slot = *ds.slot;
        hipStream_t s = slot.stream;
        MXEC_TRY(slot.shards.ensure(res_off + result_bytes(ps.p, 1, uint64_t(m))));
        auto* base = static_cast<uint8_t*>(slot.shards.p);
        // MXEC_PIPE_COPY (ops.hpp): a PUT's copies, a scrub's uploads as a GET's, never its few result bytes.
        MXEC_TRY(upload_segments(slot, s, base, up, store ? copy_waves_put(*ds.d) : copy_waves_get(*ds.d)));
        MXEC_TRY(uniform_pass(*ds.d, slot, s, {ps.p, base + res_off}, k, m, shard_size, 1, {base, 0, sa},
                              {base + sa * uint64_t(k), 0, sa}, len, nullptr));
        MXEC_TRY(download_segments(slot, s, base, down, store && copy_waves_put(*ds.d)));
        if (!store || !sha256_out) return MXEC_OK;
        // write_chunk / compute_and_write_parity digests (filesystem.rs:1070,
        // :1131), combined with every concurrent caller's verification work.
        for (int i = 0; i < k + m; ++i) staged.push_back(base + sa * uint64_t(i));
        return sha256_combined(*ds.d, slot, s, staged, len, &sha256_out[0][0]);
    });
}

}  // namespace

extern "C" {

int mxec_locate_outcome(const void* result, uint32_t* shard) {
    if (!result) return MXEC_LOCATE_MANY;
    return locate_outcome(static_cast<const mxec_locate_result*>(result), shard);
}

int mxec_encode(mxec_ctx* ctx, int k, int m, size_t shard_size, const uint8_t* const* data,
                const size_t* data_len, uint8_t* const* parity, uint8_t (*sha256_out)[32]) {
    return host_pass({Policy::Store}, ctx, k, m, shard_size, data, data_len, parity, sha256_out);
}

int mxec_verify(mxec_ctx* ctx, int k, int m, size_t shard_size, const uint8_t* const* data,
                const size_t* data_len, const uint8_t* const* parity, uint64_t* first_bad, int* consistent) {
    uint64_t rows[256];  // k + m <= 255; a caller may want the verdict alone
    uint64_t* fb = first_bad ? first_bad : rows;
    const int rc = host_pass({Policy::Compare, fb}, ctx, k, m, shard_size, data, data_len, parity, nullptr);
    if (rc == MXEC_OK && consistent)
        *consistent = std::all_of(fb, fb + m, [](uint64_t v) { return v == MXEC_VERIFY_OK; });
    return rc;
}

int mxec_locate(mxec_ctx* ctx, int k, int m, size_t shard_size, const uint8_t* const* data,
                const size_t* data_len, const uint8_t* const* parity, void* out) {
    return host_pass({Policy::Locate, out}, ctx, k, m, shard_size, data, data_len, parity, nullptr);
}

int mxec_encode_strided_device(mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                               uint64_t n_obj, const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride, const uint64_t* data_len, uint8_t* parity,
                               uint64_t parity_obj_stride, uint64_t parity_shard_stride, uint8_t* digests_dev) {
    return strided_pass({Policy::Store}, ctx, dev, stream, k, m, shard_size, n_obj,
                        {data, data_obj_stride, data_shard_stride}, data_len,
                        {parity, parity_obj_stride, parity_shard_stride}, digests_dev);
}

int mxec_encode_update_strided_device(mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                                      uint64_t n_obj, int first, int count, const uint8_t* data,
                                      uint64_t data_obj_stride, uint64_t data_shard_stride, const uint64_t* data_len,
                                      const uint8_t* parity_in, uint64_t in_obj_stride, uint64_t in_shard_stride,
                                      uint8_t* parity_out, uint64_t out_obj_stride, uint64_t out_shard_stride) {
    const Window win{first, count, {parity_in, in_obj_stride, in_shard_stride}};
    return strided_pass({Policy::Store}, ctx, dev, stream, k, m, shard_size, n_obj,
                        {data, data_obj_stride, data_shard_stride}, data_len,
                        {parity_out, out_obj_stride, out_shard_stride}, nullptr, &win);
}

int mxec_verify_strided_device(mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                               uint64_t n_obj, const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride, const uint64_t* data_len, const uint8_t* parity,
                               uint64_t parity_obj_stride, uint64_t parity_shard_stride, uint64_t* first_bad_dev) {
    return strided_pass({Policy::Compare, first_bad_dev}, ctx, dev, stream, k, m, shard_size, n_obj,
                        {data, data_obj_stride, data_shard_stride}, data_len,
                        {parity, parity_obj_stride, parity_shard_stride}, nullptr);
}

int mxec_locate_strided_device(mxec_ctx* ctx, int dev, void* stream, int k, int m, uint64_t shard_size,
                               uint64_t n_obj, const uint8_t* data, uint64_t data_obj_stride,
                               uint64_t data_shard_stride, const uint64_t* data_len, const uint8_t* parity,
                               uint64_t parity_obj_stride, uint64_t parity_shard_stride, void* out_dev) {
    return strided_pass({Policy::Locate, out_dev}, ctx, dev, stream, k, m, shard_size, n_obj,
                        {data, data_obj_stride, data_shard_stride}, data_len,
                        {parity, parity_obj_stride, parity_shard_stride}, nullptr);
}

int mxec_encode_batch_device(mxec_ctx* ctx, int dev, void* stream, const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data, const uint64_t* data_len, uint8_t* const* parity,
                             uint8_t* digests_dev) {
    return mixed_pass({Policy::Store}, ctx, dev, stream, objs, n_obj, data, data_len, parity, digests_dev);
}

int mxec_verify_batch_device(mxec_ctx* ctx, int dev, void* stream, const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data, const uint64_t* data_len, const uint8_t* const* parity,
                             uint64_t* first_bad_dev) {
    return mixed_pass({Policy::Compare, first_bad_dev}, ctx, dev, stream, objs, n_obj, data, data_len, parity, nullptr);
}

int mxec_locate_batch_device(mxec_ctx* ctx, int dev, void* stream, const mxec_object* objs, uint64_t n_obj,
                             const uint8_t* const* data, const uint64_t* data_len, const uint8_t* const* parity,
                             void* out_dev) {
    return mixed_pass({Policy::Locate, out_dev}, ctx, dev, stream, objs, n_obj, data, data_len, parity, nullptr);
}

}  // extern "C"
