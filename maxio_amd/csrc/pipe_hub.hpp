// pipe_hub.hpp -- what the host-batch calls of one device share: four
// streams, the per-call lanes and the admission of concurrent calls.
#pragma once

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

#include "runtime.hpp"

namespace mxec {

constexpr uint64_t kPoolCap = uint64_t(96) << 30;  // pool HBM per device, over the calls in flight
constexpr uint64_t kRingBuf = uint64_t(64) << 20;  // pinned ring buffer size
constexpr int kRing = 4;
constexpr int kComputeStreams = 2;  // RS stream + SHA stream (4 HW queues per process)

class PinRing {
public:
    int init(int node = -1);
    ~PinRing() {
        for (auto e : ev_)
            if (e) (void)hipEventDestroy(e);
    }
    int next() const { return next_; }
    void* ptr(int i) { return buf_[i].p; }
    hipEvent_t event(int i) { return ev_[i]; }
    // Claim the next buffer, waiting for the DMA that last used it.
    int take(int* i) {
        *i = next_;
        next_ = (next_ + 1) % kRing;
        if (busy_[*i]) MXEC_HIP(hipEventSynchronize(ev_[*i]));
        busy_[*i] = false;
        return MXEC_OK;
    }
    int mark(int i, hipStream_t s) {
        MXEC_HIP(hipEventRecord(ev_[i], s));
        busy_[i] = true;
        return MXEC_OK;
    }
    void release_all() {
        for (auto& b : busy_) b = false;
    }

private:
    PinnedBuf buf_[kRing];
    hipEvent_t ev_[kRing] = {};
    bool busy_[kRing] = {};
    int next_ = 0;
};

// Per-call resources of the pipeline (a lane): one host-batch call holds a
// lane from admission to return, so concurrent calls on one device never
// share a pool, staging ring, descriptor arena or verdict buffer.  Lanes
// are kept for later calls (their pools stay allocated: a re-size frees,
// and hipFree waits for the whole device).
struct PipeLane {
    PinRing in, out;
    DescArena arena;
    DevBuf pool, digests;
    DevBuf chain_state;  // SHA-256 chain states between pieces (host reconstruct)
    PinnedBuf flags;  // verification verdicts read back (host reconstruct)
    Slot desc_slot;  // unused ring owner for DescWriter (tables come from the arena)
    uint64_t admitted = 0;  // pool bytes this call was admitted with
    bool ready = false;
    // On a context over several NUMA nodes the staging rings and the
    // verdict buffer live on the device's node.
    int init(const Device& dev);
};

// The device's pipeline: four streams shared by every call -- H2D, D2H and
// two compute streams (the process gets 4 hardware queues; more streams
// would share them and serialise behind each other) -- and the lanes.
//
// Concurrent calls (MaxIO serves PUTs and GETs at once
// on its tokio runtime, main.rs:81): up to MXEC_PIPE_LANES calls hold lanes
// at once, admitted while the pool bytes of the calls in flight stay within
// kPoolCap (a lone call is always admitted).  Their waves interleave on the
// same streams:
//   * each call takes the compute stream fewer calls in flight use (use())
//     and queues all its kernels there, so a PUT's chains and a GET's run
//     side by side instead of one queueing behind the other, and no call's
//     RS piece waits behind another call's chain piece;
//   * a call that finds another in flight paces its enqueue (HostCopy::pace):
//     it queues a piece (or group) only after its own piece kPaceBytes back
//     is up, so the streams, which run in submission order, carry the calls'
//     work in the order it can run instead of all of one call's uploads and
//     then the other's;
//   * the SDMA watch is off while calls share the copy streams (a bracket
//     would time the other call's copies too).
struct PipeHub {
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipStream_t cs[kComputeStreams] = {};
    std::mutex mu;
    std::condition_variable cv;  // a lane came back
    std::vector<std::unique_ptr<PipeLane>> lanes;
    std::vector<PipeLane*> idle;
    int in_flight = 0;            // calls holding a lane
    uint64_t admitted_bytes = 0;  // their pool bytes
    int users[kComputeStreams] = {0, 0};  // calls in flight per compute stream (use())
    std::atomic<int> calls{0};    // in_flight, readable without the lock
    bool ready = false;
    int init(const Device& dev);
    // A lane for a call whose waves need up to `bytes` of pool (capped at
    // kPoolCap): waits while MXEC_PIPE_LANES calls are in flight, or while
    // the calls in flight hold pool bytes that would push the total past
    // kPoolCap.  Returns the lane and the bytes the call may use per wave.
    int acquire(const Device& dev, uint64_t bytes, PipeLane** out, bool* shared);
    void release(PipeLane* l);
    // The compute stream fewer calls in flight use (ties: `prefer`), counted
    // until unuse().  A call puts all its kernels there (its SHA-256 chains
    // and its RS launches; a verified GET's speculative decodes go on the
    // D2H stream): a kernel queued on a stream another call's chains use
    // waits for that call's chain pieces (a PUT's RS pieces behind a GET's
    // 4 MiB chain pieces held the PUT's chain to the GET's pace: the pair
    // ran 0.45-0.48 s, no faster than the two calls one after the other).
    int use(int prefer);
    void unuse(int c);
    // Context close (mxec_close, after the device is idle): the lanes'
    // rings, pools and events, then the streams.
    ~PipeHub();

private:
    int create_streams();
};

// A lane of the device's pipeline for the duration of one call.
class LaneScope {
public:
    LaneScope() = default;
    LaneScope(const LaneScope&) = delete;
    LaneScope& operator=(const LaneScope&) = delete;
    ~LaneScope() {
        if (lane_) hub_->release(lane_);
    }
    int open(Device& dev, uint64_t bytes);
    PipeHub& hub() { return *hub_; }
    PipeLane& lane() { return *lane_; }

private:
    std::shared_ptr<void> keep_;
    PipeHub* hub_ = nullptr;
    PipeLane* lane_ = nullptr;
};

}  // namespace mxec
