// host_copy.hpp -- how a host-batch call moves bytes between the caller's
// memory and its lane's pool: direct DMAs from page-locked memory (else
// through a ring of pinned staging buffers filled by memcpy), coalesced and
// 2D runs, CU-wave copy block tables, pacing, and the call's events.  The
// engine (SDMA or waves) is CopyWatch's choice.
#pragma once

#include <cstring>
#include <deque>
#include <utility>
#include <vector>

#include "copy_watch.hpp"
#include "kernels.hpp"
#include "pipe_hub.hpp"
#include "pipe_trace.hpp"

namespace mxec {

class HostCopy {
public:
    HostCopy(Device& d, PipeHub& h, PipeLane& l, CopyWatch& w)
        : d_(d), h2d_(h.h2d), d2h_(h.d2h), in_(l.in), out_(l.out), arena_(l.arena), slot_(l.desc_slot), watch_(w) {}
    HostCopy(const HostCopy&) = delete;
    HostCopy& operator=(const HostCopy&) = delete;
    ~HostCopy() {
        for (auto e : events_) (void)hipEventDestroy(e);
    }

    // An event of this call (no timing), destroyed when the call ends.
    int new_event(hipEvent_t* e) {
        MXEC_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        events_.push_back(*e);
        return MXEC_OK;
    }
    // Wait for this call's work queued on `s` so far (an event, not the
    // stream: calls share the streams, and a stream sync would wait for the
    // other calls' later work too).
    int sync_point(hipStream_t s);
    // While another call shares the device, a call keeps at most
    // kPaceBytes of its own uploads queued ahead of the piece (or group) it
    // has just queued (`up`: its upload is done): the shared streams run in
    // submission order, and a call that queued all its pieces at once would
    // put the other call's uploads (and what waits on them) behind all of
    // its own.  Bytes, not pieces: with two pieces each, a GET's 1 GB pieces
    // took twice the link a PUT's 512 MiB pieces got, and the starved PUT
    // chain set the pair's end.  A lone call never waits here.
    int pace(hipEvent_t up);
    void end_pacing() { paced_.clear(); }  // the wave's last piece (or group) is queued

    // Adjacent copies -- the next one starts where the last one ended, on the
    // host and on the device -- go as one DMA: an object's k data chunks are
    // usually contiguous in the request body and always in its device image
    // (and its m parity chunks likewise), so 4+2 objects take 2 copies
    // instead of 6.  In the PUT's piece-major waves (SDMA copies), copies of
    // one width at one pitch on each side -- the same piece of an object's k
    // data chunks, of its m parity chunks -- go as one 2D copy when the host
    // side is page-locked -- when the wave is upload-bound (pieces above
    // 1 MiB): PUT with digests 0.516 -> 0.457 s at 512 objects, 0.301 ->
    // 0.283 at 256 (profiles/r4/e2e_pieces/copy2d/).  At 1 MiB pieces (a
    // chain-bound wave, 128 objects) 2D copies won 2 % in the e2e tool but
    // the default bench line's leg ran 0.300 s against 0.219 with 1D copies
    // (`copy2d/bench_2d_at_1MiB_*.json`), as in round 3, so they stay 1D
    // there.  Nowhere else: in round 3 the GET group form's 2D runs of
    // whole 10 MiB shards fell from 0.113 to 0.150-0.266 s
    // (profiles/r3/pieces/).  MXEC_PIPE_COPY2D=0/1 (lab builds) forces it
    // off / on everywhere.  queue_up / queue_down collect; flush_up /
    // flush_down issue (before an event is recorded on the copy stream).
    int queue_up(uint8_t* dst, const uint8_t* src, uint64_t len) {
        if (!len) return MXEC_OK;
        up_since_pace_ += len;
        if (extend(up_run_, dst, src, len)) return MXEC_OK;
        MXEC_TRY(flush_up());
        up_run_ = Run{dst, src, len, 1, 0, 0};
        return MXEC_OK;
    }
    int flush_up() {
        const Run r = up_run_;
        up_run_ = Run{};
        if (!r.len) return MXEC_OK;
        if (r.rows == 1) return upload(r.dst, r.src, r.len);
        if (!watch_.up_by_waves() && pinned_range(r.src, (r.rows - 1) * r.spitch + r.len)) {
            if (affinity_on(d_)) {
                const void* p = r.dst;
                MXEC_TRY(affinity_check(d_, &slot_, h2d_, "pipeline upload 2d", &arena_, &p, 1));
            }
            MXEC_HIP(hipMemcpy2DAsync(r.dst, r.dpitch, r.src, r.spitch, r.len, r.rows, hipMemcpyHostToDevice, h2d_));
            ++d_.copies_2d;
            d_.copies_2d_rows += r.rows;
            return watch_.count(false, r.len * r.rows, r.rows);
        }
        for (uint64_t i = 0; i < r.rows; ++i) MXEC_TRY(upload(r.dst + i * r.dpitch, r.src + i * r.spitch, r.len));
        return MXEC_OK;
    }
    int queue_down(uint8_t* dst, const uint8_t* src, uint64_t len) {
        if (!len) return MXEC_OK;
        if (extend(down_run_, dst, src, len)) return MXEC_OK;
        MXEC_TRY(flush_down());
        down_run_ = Run{dst, src, len, 1, 0, 0};
        return MXEC_OK;
    }
    int flush_down() {
        if (!down_run_.len) return MXEC_OK;
        MXEC_TRY(flush_down_run());
        return mark_d2h();
    }
    // A piece-major wave's SDMA copies go as 2D copies (above) while set: for a Pieces2D's life.
    void pieces_2d(bool on) { pieces2d_ = on; }
    struct Pieces2D {
        HostCopy& c;
        Pieces2D(HostCopy& copy, bool on) : c(copy) { c.pieces2d_ = on; }
        ~Pieces2D() { c.pieces2d_ = false; }
    };
    // One copy now, outside the runs (a verified GET's expected digests).
    int upload(uint8_t* dst, const uint8_t* src, uint64_t len) {
        if (!len) return MXEC_OK;
        if (affinity_on(d_)) {
            const void* p = dst;
            MXEC_TRY(affinity_check(d_, &slot_, h2d_, "pipeline upload", &arena_, &p, 1));
        }
        if (wave_copy(src, dst, len, false)) {
            add_blocks(up_blks_, dst, src, len);
            return MXEC_OK;
        }
        if (pinned_range(src, len)) {
            MXEC_HIP(hipMemcpyAsync(dst, src, len, hipMemcpyHostToDevice, h2d_));
            ++d_.copies_1d;
            return watch_.count(false, len, 1);
        }
        watch_.staged(false);  // host memcpy through the ring: not an SDMA rate
        for (uint64_t off = 0; off < len; off += kRingBuf) {
            const uint64_t n = std::min(kRingBuf, len - off);
            int r;
            MXEC_TRY(in_.take(&r));
            std::memcpy(in_.ptr(r), src + off, n);
            MXEC_HIP(hipMemcpyAsync(dst + off, in_.ptr(r), n, hipMemcpyHostToDevice, h2d_));
            ++d_.copies_1d;
            MXEC_TRY(in_.mark(r, h2d_));
        }
        return MXEC_OK;
    }

    // Wave copies (MXEC_PIPE_COPY): copies from / to mxec_host_alloc memory
    // go as CU-wave copy launches (copy_kernel.hip) instead of SDMA DMAs;
    // they are collected and issued as one launch at the next point the
    // stream is waited on or marked (issue_up / issue_down).
    int issue_up() { return issue_blocks(up_blks_, false, h2d_); }
    int issue_down() {
        if (down_blks_.empty()) return MXEC_OK;
        MXEC_TRY(issue_blocks(down_blks_, true, d2h_));
        return mark_d2h();
    }
    int flush();  // end of a wave: every download has landed in the caller's memory

#ifdef MXEC_LAB
    PipeTrace& trace() { return tr_; }
#endif

private:
    struct Pending {  // ring DMA to copy out into pageable memory
        int ring;
        uint8_t* dst;
        uint64_t len;
    };
    struct Run {
        uint8_t* dst = nullptr;
        const uint8_t* src = nullptr;
        uint64_t len = 0;   // row width (0: empty)
        uint64_t rows = 0;
        uint64_t dpitch = 0, spitch = 0;
    };
    static constexpr uint64_t kPaceBytes = uint64_t(1) << 30;
    // Workgroups per copy launch: few, so the copy's host loads in flight do
    // not queue ahead of the SHA-256 chains' HBM loads (128 slowed the chains
    // 5x; 16 moves 57 GB/s alone and left the verified GET's chains alone).
    static constexpr uint32_t kCopyGrid = 16;

    bool wave_copy(const void* host, const void* dev, uint64_t len, bool down) const {
        return (down ? watch_.down_by_waves() : watch_.up_by_waves()) && copy_phase_ok(host, dev) &&
               pinned_mapped(host, len);
    }
    static void add_blocks(std::vector<CopyBlk>& v, uint8_t* dst, const uint8_t* src, uint64_t len) {
        for (uint64_t o = 0; o < len; o += kCopyBlock)
            v.push_back(CopyBlk{reinterpret_cast<uint64_t>(dst + o), reinterpret_cast<uint64_t>(src + o),
                                std::min(kCopyBlock, len - o), 0});
    }
    int issue_blocks(std::vector<CopyBlk>& v, bool to_host, hipStream_t s);
    // This call's newest work on the D2H stream, re-recorded after each of
    // its enqueues there: the call's end waits for it, not for a fresh event
    // behind the other calls' downloads queued since (a verified GET beside a
    // PUT ended with the PUT's parity downloads, ~100 ms after its own).
    int mark_d2h() {
        if (!d2h_mark_) MXEC_TRY(new_event(&d2h_mark_));
        MXEC_HIP(hipEventRecord(d2h_mark_, d2h_));
        return MXEC_OK;
    }
    bool copy2d_on() const {
#ifdef MXEC_LAB
        if (const char* e = getenv("MXEC_PIPE_COPY2D")) return atoi(e) != 0;  // lab override
#endif
        return pieces2d_;
    }
    bool extend(Run& r, uint8_t* dst, const uint8_t* src, uint64_t len) const {
        if (!r.len) return false;
        if (r.rows == 1 && r.dst + r.len == dst && r.src + r.len == src) {
            r.len += len;
            return true;
        }
        if (len != r.len || !copy2d_on()) return false;
        if (r.rows == 1) {
            if (dst < r.dst + len || src < r.src + len) return false;
            r.dpitch = uint64_t(dst - r.dst);
            r.spitch = uint64_t(src - r.src);
            r.rows = 2;
            return true;
        }
        if (dst != r.dst + r.rows * r.dpitch || src != r.src + r.rows * r.spitch) return false;
        ++r.rows;
        return true;
    }
    int flush_down_run() {
        const Run r = down_run_;
        down_run_ = Run{};
        if (!r.len) return MXEC_OK;
        if (r.rows == 1) return download(r.dst, r.src, r.len);
        if (!watch_.down_by_waves() && pinned_range(r.dst, (r.rows - 1) * r.dpitch + r.len)) {
            if (affinity_on(d_)) {
                const void* p = r.src;
                MXEC_TRY(affinity_check(d_, &slot_, d2h_, "pipeline download 2d", &arena_, &p, 1));
            }
            MXEC_HIP(hipMemcpy2DAsync(r.dst, r.dpitch, r.src, r.spitch, r.len, r.rows, hipMemcpyDeviceToHost, d2h_));
            ++d_.copies_2d;
            d_.copies_2d_rows += r.rows;
            return watch_.count(true, r.len * r.rows, r.rows);
        }
        for (uint64_t i = 0; i < r.rows; ++i) MXEC_TRY(download(r.dst + i * r.dpitch, r.src + i * r.spitch, r.len));
        return MXEC_OK;
    }
    // Copy out the pending ring buffer the next take() will reuse.
    int drain_next();
    int download(uint8_t* dst, const uint8_t* src, uint64_t len) {
        if (!len) return MXEC_OK;
        if (affinity_on(d_)) {
            const void* p = src;
            MXEC_TRY(affinity_check(d_, &slot_, d2h_, "pipeline download", &arena_, &p, 1));
        }
        if (wave_copy(dst, src, len, true)) {
            add_blocks(down_blks_, dst, src, len);
            return MXEC_OK;
        }
        if (pinned_range(dst, len)) {
            MXEC_HIP(hipMemcpyAsync(dst, src, len, hipMemcpyDeviceToHost, d2h_));
            ++d_.copies_1d;
            return watch_.count(true, len, 1);
        }
        watch_.staged(true);
        for (uint64_t off = 0; off < len; off += kRingBuf) {
            const uint64_t n = std::min(kRingBuf, len - off);
            MXEC_TRY(drain_next());
            int r;
            MXEC_TRY(out_.take(&r));
            MXEC_HIP(hipMemcpyAsync(out_.ptr(r), src + off, n, hipMemcpyDeviceToHost, d2h_));
            ++d_.copies_1d;
            MXEC_TRY(out_.mark(r, d2h_));
            pend_.push_back(Pending{r, dst + off, n});
        }
        return MXEC_OK;
    }

    Device& d_;
    const hipStream_t h2d_, d2h_;
    PinRing& in_;
    PinRing& out_;
    DescArena& arena_;
    Slot& slot_;
    CopyWatch& watch_;
    std::vector<Pending> pend_;
    std::vector<hipEvent_t> events_;
    std::deque<std::pair<hipEvent_t, uint64_t>> paced_;
    uint64_t up_since_pace_ = 0;  // bytes queue_up took since the last pace()
    std::vector<CopyBlk> up_blks_, down_blks_;
    hipEvent_t d2h_mark_ = nullptr;
    Run up_run_, down_run_;
    bool pieces2d_ = false;
#ifdef MXEC_LAB
    PipeTrace tr_;
#endif
};

}  // namespace mxec
