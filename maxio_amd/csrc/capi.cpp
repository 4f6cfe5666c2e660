// capi.cpp — extern "C" entry points of include/maxio_ec.h: context, stats,
// page-locked host memory and SHA-256 batches (the parity pass, encode /
// verify / locate, is parity_pass.cpp; the reconstructs are reconstruct.cpp).
// No exception crosses the ABI.
#include <algorithm>
#include <cctype>
#include <fstream>
#include <string>

#include "../../include/maxio_ec.h"
#include "kernels.hpp"
#include "ops.hpp"

using namespace mxec;

extern "C" {

const char* mxec_version(void) {
#ifdef MXEC_LAB
    return "maxio_ec 0.1.0 (gfx950, lab build)";
#else
    return "maxio_ec 0.1.0 (gfx950)";
#endif
}

const char* mxec_strerror(int code) {
    switch (code) {
        case MXEC_OK: return "ok";
        case MXEC_E_TOO_FEW_SHARDS: return "The number of provided shards is smaller than the one in codec";
        case MXEC_E_TOO_MANY_SHARDS: return "The number of provided shards is greater than the one in codec";
        case MXEC_E_TOO_FEW_DATA_SHARDS: return "The number of provided data shards is smaller than the one in codec";
        case MXEC_E_TOO_MANY_DATA_SHARDS: return "The number of provided data shards is greater than the one in codec";
        case MXEC_E_TOO_FEW_PARITY_SHARDS: return "The number of provided parity shards is smaller than the one in codec";
        case MXEC_E_TOO_MANY_PARITY_SHARDS: return "The number of provided parity shards is greater than the one in codec";
        case MXEC_E_TOO_FEW_BUFFER_SHARDS: return "The number of provided buffer shards is smaller than the number of parity shards in codec";
        case MXEC_E_TOO_MANY_BUFFER_SHARDS: return "The number of provided buffer shards is greater than the number of parity shards in codec";
        case MXEC_E_INCORRECT_SHARD_SIZE: return "At least one of the provided shards is not of the correct size";
        case MXEC_E_TOO_FEW_SHARDS_PRESENT: return "The number of shards present is smaller than number of parity shards, cannot reconstruct missing shards";
        case MXEC_E_EMPTY_SHARD: return "The first shard provided is of zero length";
        case MXEC_E_INVALID_SHARD_FLAGS: return "The number of flags does not match the total number of shards";
        case MXEC_E_INVALID_INDEX: return "The data shard index provided is greater or equal to the number of data shards in codec";
        case MXEC_E_SINGULAR_MATRIX: return "singular matrix";
        case MXEC_E_TOO_MANY_SHARDS_255: return "too many shards (> 255, GF(2^8) limit)";
        case MXEC_E_INVALID_ARG: return "invalid argument";
        case MXEC_E_DEVICE: return "HIP device error";
        case MXEC_E_OOM: return "out of memory";
        case MXEC_E_NO_DEVICE: return "no HIP device";
        case MXEC_E_IO: return "IO error";
        case MXEC_E_INTEGRITY: return "integrity error";
        case MXEC_E_JSON: return "JSON error";
        default: return "unknown error";
    }
}

const char* mxec_last_error(void) { return last_error(); }

int mxec_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace {

// NUMA node of HIP device `dev` (sysfs, through its PCI bus id), or -1.
int device_numa_node(int dev) {
    char bus[64] = {};
    if (hipDeviceGetPCIBusId(bus, int(sizeof bus), dev) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char& c : bus) c = char(std::tolower(static_cast<unsigned char>(c)));
    std::ifstream f(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
    int node = -1;
    return f >> node ? node : -1;
}

// The node all of the context's devices sit on, or -1 (unknown or several).
int ctx_numa_node(const mxec_ctx* ctx) {
    int node = -1;
    for (const auto& d : ctx->c.devs) {
        const int n = d->numa_node;
        if (n < 0 || (node >= 0 && n != node)) return -1;
        node = n;
    }
    return node;
}

}  // namespace

namespace {
// The one open path.  `logical` > 1 (mxec_open_test only) opens every
// selected device that many times, each copy with its own slots, streams,
// arenas, combiner and pipeline, so the multi-device paths (per-device
// workers, round robin, error aggregation) run on a one-GPU box.
mxec_ctx* open_ctx(uint32_t device_mask, int streams_per_device, const Knobs& kn) {
    try {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            set_error(MXEC_E_NO_DEVICE, "no HIP device visible");
            return nullptr;
        }
        if (streams_per_device < 1) streams_per_device = 1;
        const int logical = kn.test_logical_devices;
        auto* ctx = new mxec_ctx();
        ctx->c.knobs = kn;
        for (int dl = 0; dl < n * logical && dl < 32 * logical; ++dl) {
            const int d = dl / logical;
            if (device_mask && !(device_mask & (1u << d))) continue;
            auto dev = std::make_unique<Device>();
            dev->id = d;
            dev->kn = &ctx->c.knobs;
            if (hipSetDevice(d) != hipSuccess) continue;
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && cus > 0)
                dev->n_cus = cus;
            // test-only logical copies pretend to sit on two nodes, so the
            // host pipeline's NUMA dealing runs on a one-card box
            dev->numa_node = logical > 1 ? (dl % logical) % 2 : device_numa_node(d);
            bool ok = true;
            for (int s = 0; s < streams_per_device; ++s) {
                auto slot = std::make_unique<Slot>();
                slot->owner = dev.get();
                if (hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking) != hipSuccess) {
                    ok = false;
                    break;
                }
                affinity_tag(slot->stream, dev.get());
                // Descriptor ring entries at their 1 MiB floor now, so the
                // first calls on each slot do not allocate (and a later
                // re-size, which frees and so waits for the device, is rare).
                for (auto& rb : slot->ring)
                    if (rb.host.grow(1) || rb.dev.grow(1)) {
                        ok = false;
                        break;
                    }
                if (!ok) {
                    slot_destroy(*slot);
                    break;
                }
                dev->slots.push_back(std::move(slot));
            }
            if (ok && pipe_open(*dev) != MXEC_OK) {
                for (auto& sl : dev->slots) slot_destroy(*sl);
                ok = false;
            }
            if (ok) ctx->c.devs.push_back(std::move(dev));
        }
        if (ctx->c.devs.empty()) {
            delete ctx;
            set_error(MXEC_E_NO_DEVICE, "no selected HIP device could be opened");
            return nullptr;
        }
        bool multi = false;
        for (const auto& d : ctx->c.devs)
            multi = multi || (d->numa_node >= 0 && d->numa_node != ctx->c.devs[0]->numa_node);
        for (auto& d : ctx->c.devs) d->ctx_multi_node = multi && d->numa_node >= 0;
        return ctx;
    } catch (...) {
        set_error(MXEC_E_OOM, "context allocation failed");
        return nullptr;
    }
}
}  // namespace

// Every documented setting is read once, here (knobs.hpp).
mxec_ctx* mxec_open(uint32_t device_mask, int streams_per_device) {
    return open_ctx(device_mask, streams_per_device, read_knobs());
}

// Test-only settings come as arguments, never from the environment, so no
// variable a production host may carry can make one card pose as several
// devices, cap the RS grid or shrink the coefficient arena.
mxec_ctx* mxec_open_test(uint32_t device_mask, int streams_per_device, int logical_devices, uint32_t rs_grid_cap,
                         uint64_t coef_arena_bytes) {
    Knobs kn = read_knobs();
    if (logical_devices < 1 || logical_devices > 8 || coef_arena_bytes > (uint64_t(64) << 20) ||
        rs_grid_cap > (1u << 30)) {
        set_error(MXEC_E_INVALID_ARG, "mxec_open_test: logical_devices 1..8, rs_grid_cap <= 2^30, "
                                      "coef_arena_bytes <= 64 MiB");
        return nullptr;
    }
    kn.test_logical_devices = logical_devices;
    kn.test_rs_grid = rs_grid_cap;
    kn.test_coef_arena = coef_arena_bytes & ~uint64_t(3);
    return open_ctx(device_mask, streams_per_device, kn);
}

void mxec_close(mxec_ctx* ctx) {
    if (!ctx) return;
    async_shutdown(ctx->c);  // every queued *_async call finishes first
    if (ctx->c.knobs.debug_affinity) affinity_report();
    for (auto& d : ctx->c.devs) {
        (void)hipSetDevice(d->id);
        (void)hipDeviceSynchronize();
        // The host pipeline's lanes (pinned rings, pools, descriptor arenas,
        // events) and its four streams, and the combiner's streams, go first
        // and explicitly, while the device is idle.
        {
            std::lock_guard<std::mutex> g(d->pipe_mu);
            d->pipe.reset();
        }
        {
            std::lock_guard<std::mutex> g(d->comb_mu);
            d->comb.reset();
        }
        rs_grid_release(*d);
        coef_release(*d);
        for (auto& s : d->slots) slot_destroy(*s);
    }
    delete ctx;
}

int mxec_ctx_device_count(const mxec_ctx* ctx) { return ctx ? int(ctx->c.devs.size()) : 0; }

int mxec_ctx_device_id(const mxec_ctx* ctx, int i) {
    if (!ctx || i < 0 || i >= int(ctx->c.devs.size())) return -1;
    return ctx->c.devs[size_t(i)]->id;
}

int mxec_ctx_pipe_stats(mxec_ctx* ctx, int dev, uint64_t* out, int n) {
    if (!ctx || dev < 0 || dev >= int(ctx->c.devs.size()) || !out || n < 0)
        return set_error(MXEC_E_INVALID_ARG, "mxec_ctx_pipe_stats: no such device or no output");
    const Device& d = *ctx->c.devs[size_t(dev)];
    const uint64_t v[MXEC_PIPE_STAT_COUNT] = {d.copies_1d.load(),        d.copies_2d.load(),
                                              d.copies_2d_rows.load(),   d.copy_wave_blocks.load(),
                                              d.sdma_probes.load(),      d.sdma_slow_verdicts.load(),
                                              d.verify_waves.load(),     d.verify_groups.load(),
                                              d.sdma_last_mbps.load(),   d.sdma_down_probes.load(),
                                              d.sdma_down_slow_verdicts.load(), d.sdma_down_last_mbps.load(),
                                              d.pipe_calls.load(),       d.pipe_calls_shared.load(),
                                              d.spec_pieces.load(),      d.spec_redos.load(),
                                              d.pace_waits.load()};
    const int k = std::min(n, int(MXEC_PIPE_STAT_COUNT));
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

int mxec_ctx_combiner_stats(mxec_ctx* ctx, int i, uint64_t* launches, uint64_t* messages) {
    if (!ctx || i < 0 || i >= int(ctx->c.devs.size()) || !launches || !messages)
        return set_error(MXEC_E_INVALID_ARG, "invalid argument");
    combiner_stats(*ctx->c.devs[size_t(i)], launches, messages);
    return MXEC_OK;
}

int mxec_ctx_coef_stats(mxec_ctx* ctx, int dev, uint64_t* recycles, uint64_t* relaunches, uint64_t* fence_waits) {
    if (!ctx || dev < 0 || dev >= int(ctx->c.devs.size()) || !recycles || !relaunches)
        return set_error(MXEC_E_INVALID_ARG, "invalid argument");
    Device& d = *ctx->c.devs[size_t(dev)];
    std::lock_guard<std::mutex> g(d.coef_mu);
    *recycles = d.coef_recycles;
    *relaunches = d.coef_relaunches;
    if (fence_waits) *fence_waits = d.coef_fence_waits;
    return MXEC_OK;
}

int mxec_ctx_rs_grid(mxec_ctx* ctx, int dev, int k, int m, uint64_t shard_size) {
    if (!ctx || dev < 0 || dev >= int(ctx->c.devs.size()) || k < 1 || m < 1)
        return set_error(MXEC_E_INVALID_ARG, "invalid argument");
    return guarded([&] { return rs_grid_in_use(*ctx->c.devs[size_t(dev)], k, m, shard_size); });
}


// Page-locked memory on the NUMA node of the context's GPUs with
// MXEC_HOST_NUMA=1 (default: wherever the calling thread's policy puts it).  The pages are placed when
// hipHostMalloc pins them, so the thread's policy is set to that node around
// the call (hipHostMallocNumaUser) and restored after; if the node is unknown
// or the policy calls are refused, the allocation is the plain one.  A
// process may run on every core of a two-socket host, and a DMA from the far
// socket's memory crosses the socket link.
namespace {
void* host_alloc_on(size_t bytes, int node) {
    void* p = nullptr;
    if (host_malloc_on_node(&p, bytes, node, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        set_error(MXEC_E_OOM, "pinned host allocation failed");
        return nullptr;
    }
    pinned_register(p, bytes);
    return p;
}
}  // namespace

void* mxec_host_alloc(mxec_ctx* ctx, size_t bytes) {
    if (!ctx || bytes == 0) return nullptr;
    return host_alloc_on(bytes, ctx->c.knobs.host_numa ? ctx_numa_node(ctx) : -1);  // opt-in until measured
}

// On a two-socket host a context spans both nodes and mxec_host_alloc has no
// one node to pick (ctx_numa_node gives up): a request body meant for device
// `dev` goes on that device's node, whatever MXEC_HOST_NUMA says, and the
// host batch calls then deal the object to a device on that node
// (deal.hpp deal_objects_numa).
void* mxec_host_alloc_device(mxec_ctx* ctx, int dev, size_t bytes) {
    if (!ctx || bytes == 0 || dev < 0 || dev >= int(ctx->c.devs.size())) {
        set_error(MXEC_E_INVALID_ARG, "mxec_host_alloc_device: no such device or zero bytes");
        return nullptr;
    }
    return host_alloc_on(bytes, ctx->c.devs[size_t(dev)]->numa_node);
}

void mxec_host_free(mxec_ctx* ctx, void* p) {
    (void)ctx;
    if (!p) return;
    pinned_unregister(p);
    (void)hipHostFree(p);
}

int mxec_rs_check(int k, int m) { return rs_check(k, m); }

int mxec_rs_parity_matrix(int k, int m, uint8_t* out) {
    return guarded([&] {
        int rc = rs_check(k, m);
        if (rc) return rc;
        if (!out) return set_error(MXEC_E_INVALID_ARG, "null output");
        auto mat = rs_matrix(k, m);
        if (!mat) return set_error(MXEC_E_SINGULAR_MATRIX, "matrix construction failed");
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < k; ++j) out[size_t(i) * k + j] = mat->at(k + i, j);
        return MXEC_OK;
    });
}

int mxec_sha256_batch(mxec_ctx* ctx, const uint8_t* const* bufs, const size_t* lens, size_t n,
                      uint8_t (*out)[32]) {
    return guarded([&] {
        if (n == 0) return MXEC_OK;
        if (!bufs || !lens || !out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        DevScope ds;
        MXEC_TRY(ds.open(ctx, -1));
        Slot& slot = *ds.slot;
        hipStream_t s = slot.stream;
        uint64_t total = 0;
        std::vector<uint64_t> off(n);
        for (size_t i = 0; i < n; ++i) {
            off[i] = total;
            total += round_up(lens[i] ? lens[i] : 1, kSlotAlign);
        }
        MXEC_TRY(slot.shards.ensure(total));
        MXEC_TRY(slot.digests.grow(n * 32));
        auto* base = static_cast<uint8_t*>(slot.shards.p);
        std::vector<const uint8_t*> ptrs(n);
        std::vector<uint64_t> l(n);
        std::vector<UploadSeg> segs;
        segs.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            if (lens[i]) segs.push_back({off[i], bufs[i], lens[i]});
            ptrs[i] = base + off[i];
            l[i] = lens[i];
        }
        MXEC_TRY(upload_segments(slot, s, base, segs, copy_waves_get(*ds.d)));
        MXEC_TRY(slot_wait(slot, s));  // uploads done: the combiner hashes on its own stream
        return sha256_combined(*ds.d, slot, s, ptrs, l, &out[0][0]);
    });
}

int mxec_sha256_batch_device(mxec_ctx* ctx, int dev, void* stream, const uint8_t* const* bufs,
                             const uint64_t* lens, uint64_t n, uint8_t* digests_dev) {
    return guarded([&] {
        if (n == 0) return MXEC_OK;
        if (!bufs || !lens || !digests_dev) return set_error(MXEC_E_INVALID_ARG, "null argument");
        for (uint64_t i = 0; i < n; ++i)
            if (!bufs[i]) return set_error(MXEC_E_INVALID_ARG, "null message pointer " + std::to_string(i));
        DevScope ds;
        MXEC_TRY(ds.open(ctx, dev));
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the HIP null stream
        std::vector<const uint8_t*> p(bufs, bufs + n);
        std::vector<uint64_t> l(lens, lens + n);
        return run_sha(*ds.d, *ds.slot, s, p, l, digests_dev, nullptr, nullptr);
    });
}

}  // extern "C"
