// pipe_hub.cpp -- the host pipeline's streams, lanes and admission (pipe_hub.hpp).
#include "pipe_hub.hpp"

#include "ops.hpp"

namespace mxec {

int PinRing::init(int node) {
    for (int i = 0; i < kRing; ++i) {
        buf_[i].node = node;
        MXEC_TRY(buf_[i].ensure(kRingBuf));
        MXEC_HIP(hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming));
    }
    return MXEC_OK;
}

int PipeLane::init(const Device& dev) {
    if (ready) return MXEC_OK;
    desc_slot.owner = &dev;
    arena.owner = &dev;
    const int node = dev.ctx_multi_node ? dev.numa_node : -1;
    flags.node = node;
    MXEC_TRY(in.init(node));
    MXEC_TRY(out.init(node));
    ready = true;
    return MXEC_OK;
}

int PipeHub::init(const Device& dev) {
    if (ready) return MXEC_OK;
    MXEC_TRY(create_streams());
    affinity_tag(h2d, &dev);
    affinity_tag(d2h, &dev);
    for (auto s : cs) affinity_tag(s, &dev);
    ready = true;
    return MXEC_OK;
}

int PipeHub::acquire(const Device& dev, uint64_t bytes, PipeLane** out, bool* shared) {
    const int max_lanes = dev.kn ? dev.kn->pipe_lanes : 4;
    bytes = std::min(bytes, kPoolCap);
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] {
        return in_flight == 0 || (in_flight < max_lanes && admitted_bytes + bytes <= kPoolCap);
    });
    if (in_flight == 0)  // nothing of ours runs: buffers retired by re-sizes can go now
        for (auto& ln : lanes) ln->pool.free_retired();
    PipeLane* l = nullptr;
    if (!idle.empty()) {
        // the idle lane with the largest pool (fewest re-sizes)
        size_t best = 0;
        for (size_t i = 1; i < idle.size(); ++i)
            if (idle[i]->pool.cap > idle[best]->pool.cap) best = i;
        l = idle[best];
        idle.erase(idle.begin() + long(best));
    } else {
        lanes.emplace_back(new PipeLane());
        l = lanes.back().get();
    }
    *shared = in_flight > 0;
    ++in_flight;
    calls.store(in_flight);
    admitted_bytes += bytes;
    l->admitted = bytes;
    lk.unlock();
    const int rc = l->init(dev);
    if (rc != MXEC_OK) release(l);
    *out = rc == MXEC_OK ? l : nullptr;
    return rc;
}

void PipeHub::release(PipeLane* l) {
    {
        std::lock_guard<std::mutex> g(mu);
        --in_flight;
        calls.store(in_flight);
        admitted_bytes -= l->admitted;
        l->admitted = 0;
        idle.push_back(l);
    }
    cv.notify_all();
}

int PipeHub::use(int prefer) {
    std::lock_guard<std::mutex> g(mu);
    const int c = users[1 - prefer] < users[prefer] ? 1 - prefer : prefer;
    ++users[c];
    return c;
}

void PipeHub::unuse(int c) {
    std::lock_guard<std::mutex> g(mu);
    --users[c];
}

// Plain non-blocking streams at the highest stream priority, created when
// the context opens (pipe_open): HIP serves a process's streams from
// GPU_MAX_HW_QUEUES (4) hardware queues per priority, and normal-priority
// streams -- the context's slots, the table stream, torch's -- already share
// them.  Two of the pipeline's streams on one queue serialise across it:
// with a GET's chain stream and the D2H stream on one queue every hash piece
// waited for the previous piece's speculative decode and download (26 ms per
// 1 MiB piece against 19; profiles/r6/).  The high-priority pool is empty at
// mxec_open, so the four streams get four queues; the compute streams are
// created first, so the SHA-256 combiner's high-priority streams (created
// on its first use) share the compute streams' queues, never a copy
// stream's.  Measured and not kept (lab settings, since removed): the copy
// streams on a few masked CUs and the compute streams on the rest (no
// different from unmasked at the wave copies' 16 workgroups,
// profiles/r4/get_stall/), the compute streams on complementary halves of
// the CUs, a CU mask of every CU for a hardware queue per stream, and round
// 5's normal-priority streams.
int PipeHub::create_streams() {
    int least = 0, greatest = 0;
    MXEC_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (auto& s : cs) MXEC_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
    MXEC_HIP(hipStreamCreateWithPriority(&h2d, hipStreamNonBlocking, greatest));
    MXEC_HIP(hipStreamCreateWithPriority(&d2h, hipStreamNonBlocking, greatest));
    return MXEC_OK;
}

PipeHub::~PipeHub() {
    lanes.clear();
    for (auto s : cs)
        if (s) {
            affinity_untag(s);
            (void)hipStreamDestroy(s);
        }
    affinity_untag(h2d);
    affinity_untag(d2h);
    if (h2d) (void)hipStreamDestroy(h2d);
    if (d2h) (void)hipStreamDestroy(d2h);
}

int LaneScope::open(Device& dev, uint64_t bytes) {
    {
        std::lock_guard<std::mutex> g(dev.pipe_mu);
        if (!dev.pipe) dev.pipe = std::make_shared<PipeHub>();
        keep_ = dev.pipe;
    }
    hub_ = static_cast<PipeHub*>(keep_.get());
    {
        std::lock_guard<std::mutex> g(dev.pipe_mu);  // stream creation, once
        MXEC_TRY(hub_->init(dev));
    }
    bool shared = false;
    MXEC_TRY(hub_->acquire(dev, bytes, &lane_, &shared));
    ++dev.pipe_calls;
    if (shared) ++dev.pipe_calls_shared;
    return MXEC_OK;
}

// The device's pipeline hub and its four streams, at context open (their
// hardware queues depend on what the process created before them).
int pipe_open(Device& dev) {
    std::lock_guard<std::mutex> g(dev.pipe_mu);
    if (!dev.pipe) dev.pipe = std::make_shared<PipeHub>();
    return static_cast<PipeHub*>(dev.pipe.get())->init(dev);
}

}  // namespace mxec
