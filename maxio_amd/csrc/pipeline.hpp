// pipeline.hpp -- what the host-memory batch calls share: the PUT
// (pipeline_put.cpp) and the GET (pipeline_get.cpp) spread a batch over every
// device of the context and run each device's share in waves.
//
// Per device (one host thread each; objects dealt round-robin over devices
// when the batch is uniform, by bytes when it is mixed, deal.hpp):
//   * an HBM object pool holds a whole wave of objects (k+m shard slots and
//     k+m digests each, up to kPoolCap bytes), so the latency-bound SHA-256
//     launches of many groups run concurrently instead of waiting on a small
//     staging window (288 GB of HBM makes this the cheap resource);
//   * copies go on dedicated H2D and D2H streams (host_copy.hpp), kernels on
//     the call's compute stream right behind the uploads they read;
//   * descriptor tables come from a per-wave arena so nothing throttles the
//     launches in flight.
#pragma once

#include <algorithm>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include <sys/syscall.h>
#include <unistd.h>

#include "deal.hpp"
#include "host_copy.hpp"
#include "ops.hpp"
#include "piece_grid.hpp"
#include "wave_cut.hpp"

namespace mxec {

constexpr uint64_t kAlign = 256;
constexpr uint64_t kGroupBytes = uint64_t(256) << 20;  // input bytes per group
inline uint64_t rup(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// NUMA node of the page at p (get_mempolicy MPOL_F_NODE | MPOL_F_ADDR), or -1.
inline int page_node(const void* p) {
    if (!p) return -1;
    int node = -1;
    return syscall(SYS_get_mempolicy, &node, nullptr, 0, const_cast<void*>(p), 3 /* MPOL_F_NODE | MPOL_F_ADDR */) == 0
               ? node
               : -1;
}

// Device of each object of a host batch: o mod D / by bytes (deal_objects);
// on a context over several NUMA nodes, by the node of each object's first
// host page (`first[o]`), balanced (deal_objects_numa).
inline std::vector<uint32_t> deal_batch(const Ctx& c, const std::vector<uint64_t>& bytes,
                                        const std::vector<const void*>& first) {
    const uint32_t D = uint32_t(c.devs.size());
    if (D <= 1 || !c.devs[0]->ctx_multi_node) return deal_objects(bytes, D);
    std::vector<int> dev_node(D), node(bytes.size(), -1);
    for (uint32_t d = 0; d < D; ++d) dev_node[d] = c.devs[d]->numa_node;
    for (size_t o = 0; o < bytes.size(); ++o) node[o] = page_node(first[o]);
    return deal_objects_numa(bytes, node, dev_node);
}

// One host-batch call's share of one device: the device, the lane it holds,
// the compute stream it queues its kernels on, its copies and their watch.
// The PUT and the GET derive their waves from it.
class PipeCall {
public:
    // prefer: the compute stream taken when both are equally used (PipeHub::use).
    PipeCall(Device& d, PipeHub& h, PipeLane& l, int prefer)
        : d_(d), hub_(h), h2d_(h.h2d), d2h_(h.d2h), cs_(h.cs), arena_(l.arena), pool_(l.pool), scratch_(l.digests),
          state_(l.chain_state), flags_(l.flags), slot_(l.desc_slot), cap_(std::max<uint64_t>(l.admitted, 1)),
          cs_idx_(h.use(prefer)), watch_(d, h.h2d, h.d2h, h.calls), copy_(d, h, l, watch_) {}
    PipeCall(const PipeCall&) = delete;
    PipeCall& operator=(const PipeCall&) = delete;
    // The compute stream goes back first, then the call's events (members).
    ~PipeCall() { hub_.unuse(cs_idx_); }

protected:
    // wave(o0, o1) over the waves of objs (wave_cut.hpp), each with its pool and arena in place.
    template <class Obj, class Wave>
    int run_waves(std::vector<Obj>& objs, Wave&& wave) {
        watch_.start_call();
        std::vector<uint64_t> pool(objs.size()), desc(objs.size());
        for (size_t o = 0; o < objs.size(); ++o) {
            pool[o] = objs[o].bytes();
            desc[o] = objs[o].desc_bytes();
        }
        const WaveCuts cuts = cut_waves(pool, desc, cap_);
        for (size_t o = 0; o < objs.size(); ++o) objs[o].pool_off = cuts.pool_off[o];
        for (const auto& w : cuts.waves) {
            MXEC_TRY(pool_.replace(w.pool));  // no free while other calls run (retired until idle)
            MXEC_TRY(arena_.reserve(w.arena));
            MXEC_TRY(wave(w.begin, w.end));
        }
        return watch_.end_call();
    }

    // Piece size of a piece-major wave (MXEC_PIPE_PIECE_MB; unset = per
    // wave): small pieces start the chains early, but each piece of each
    // chunk is its own copy, and 1 MiB copies move ~33 GB/s where 4 MiB ones
    // move ~43 (PUT with digests, 512 x 4+2 x 10 MiB: 0.645 s at 1 MiB,
    // 0.557 at 2, 0.503 at 4; 128 objects: 0.218 / 0.227 / 0.246 s,
    // profiles/r4/e2e_pieces/).  So a wave takes the smallest piece whose
    // upload, at that piece's copy rate, still fits inside the longest chain
    // (the wave's floor either way), else 4 MiB.
    //
    // A chain-bound verified GET wave (its upload fits inside its longest
    // chain) also ramps its first pieces up from 256 KiB (piece_ramp_,
    // PieceGrid): it ends about one chain after its first piece is up, so a
    // smaller first piece ends it sooner -- 128 x 4+2 x 10 MiB 0.2406 s
    // against 0.2475 with its uploads by waves (rec_wave).  The PUT with
    // digests lost to the same ramp (0.214-0.223 against 0.2033 by SDMA;
    // profiles/r5/get_groups/ramp_ab_final_r5ab.jsonl), and an upload-bound
    // wave loses to the extra copies (512 objects: 0.606 against 0.588,
    // ramp_*_r5u.jsonl), so the PUT's wave() clears it and only chain-bound
    // waves set it.
    //
    // While other calls share the device, they share its upload link too: the
    // wave's upload is weighed as if it were the calls-in-flight times larger
    // (a PUT with digests beside a verified GET, 128 x 4+2 x 10 MiB each:
    // 10.7 GB over the link against a 191 ms chain, upload-bound, so 4 MiB
    // pieces and 2D copies instead of 1 MiB ones at ~33 GB/s).
    uint64_t piece_bytes(uint64_t upload_bytes, uint64_t longest) {
        piece_ramp_ = 0;
        if (!d_.kn) return uint64_t(1) << 20;
        if (!d_.kn->pipe_piece_auto) return d_.kn->pipe_piece;
        const int calls = std::max(1, hub_.calls.load());
        upload_bytes *= uint64_t(calls);
        const double chain_s = double(longest / 64) * kShaLagUsPerBlock * 1e-6;
        static constexpr struct {
            uint64_t bytes;
            double gbps;  // sustained H2D rate of copies this size, measured (above)
        } kSteps[] = {{uint64_t(1) << 20, 33.0}, {uint64_t(2) << 20, 38.0}};
        for (const auto& s : kSteps)
            if (double(upload_bytes) / (s.gbps * 1e9) <= chain_s) {
                piece_ramp_ = uint64_t(256) << 10;
                return s.bytes;
            }
        // Upload-bound.  A wave that shares the link still ramps: its first
        // pieces go up between the other call's, so both calls' chains start
        // early (without, a GET's first 4 MiB piece -- 2 GB for 128 x 4+2 --
        // held a PUT's first piece back 45 ms, and the PUT's chain set the
        // pair's end).
        if (calls > 1) {
            piece_ramp_ = uint64_t(256) << 10;
            return uint64_t(2) << 20;  // pieces the other call's can interleave with (2D copies above 1 MiB)
        }
        return uint64_t(4) << 20;
    }
    // A wave sized while it had the device to itself (1 MiB pieces: its
    // upload fit inside its chains) goes on in 2 MiB pieces, 2D copies, once
    // another call shares the link -- piece_bytes' choice had it known (a
    // PUT with digests admitted just before a verified GET otherwise kept
    // its ~33 GB/s 1 MiB copies through the pair and ended ~90 ms after the
    // GET).
    void widen_if_shared(PieceGrid& grid, uint64_t pc) {
        static constexpr uint64_t kShared = uint64_t(2) << 20;
        if (!d_.kn || !d_.kn->pipe_piece_auto || pc < grid.starts.size() || grid.P >= kShared || !watch_.shared_now())
            return;
        grid.widen(pc, kShared);
        copy_.pieces_2d(!watch_.up_by_waves());
    }
    // The lag quad form's capacity: a wave of more messages takes the group form.
    uint64_t lag_capacity() const { return uint64_t(kShaLagMsgs) * uint64_t(d_.n_cus ? d_.n_cus : 256); }
#ifdef MXEC_LAB
    PipeTrace& trace() { return copy_.trace(); }
#endif

    Device& d_;
    PipeHub& hub_;
    const hipStream_t h2d_, d2h_;
    hipStream_t* const cs_;
    DescArena& arena_;
    DevBuf& pool_;
    DevBuf& scratch_;  // the wave's digests, message order
    DevBuf& state_;    // chain states of a piece-major verification
    PinnedBuf& flags_;
    Slot& slot_;
    const uint64_t cap_;  // pool bytes per wave (the lane's admission)
    const int cs_idx_;    // the compute stream this call's kernels run on (PipeHub::use)
    uint64_t piece_ramp_ = 0;  // first piece of the current wave's ramp (0: none)
    CopyWatch watch_;
    HostCopy copy_;
};

// run(device, hub, lane, per[d]) for every device d with objects in per[d],
// one worker per device.  Every thread is joined on every path (a joinable
// std::thread destroyed during unwinding would terminate the process), and
// no exception leaves a worker.  Returns the first failing device's error.
template <class Obj, class Run>
int for_each_device(Ctx& c, std::vector<std::vector<Obj>>& per, Run&& run) {
    const size_t D = per.size();
    std::vector<int> rcs(D, MXEC_OK);
    std::vector<std::string> errs(D);
    struct Joiner {
        std::vector<std::thread> th;
        ~Joiner() {
            for (auto& t : th)
                if (t.joinable()) t.join();
        }
    } j;
    auto work = [&](size_t d) {
        try {
            Device& dev = *c.devs[d];
            rcs[d] = [&]() -> int {
                MXEC_HIP(hipSetDevice(dev.id));
                uint64_t bytes = 0;
                for (const auto& h : per[d]) bytes += h.bytes();
                LaneScope lane;
                MXEC_TRY(lane.open(dev, bytes));
                return run(dev, lane.hub(), lane.lane(), per[d]);
            }();
            if (rcs[d] != MXEC_OK) errs[d] = last_error();
        } catch (const std::bad_alloc&) {
            rcs[d] = MXEC_E_OOM;
            errs[d] = "host allocation failed";
        } catch (const std::exception& e) {
            rcs[d] = MXEC_E_INVALID_ARG;
            errs[d] = e.what();
        }
    };
    for (size_t d = 0; d < D; ++d) {
        if (per[d].empty()) continue;
        try {
            j.th.emplace_back(work, d);
        } catch (const std::system_error&) {
            work(d);  // no thread to be had: run this device's share here
        }
    }
    for (auto& t : j.th) t.join();
    for (size_t d = 0; d < D; ++d)
        if (rcs[d] != MXEC_OK) return set_error(rcs[d], errs[d]);
    return MXEC_OK;
}

}  // namespace mxec
