// copy_watch.hpp -- which engine a host-batch call's copies of
// mxec_host_alloc memory take (SDMA DMAs or CU-wave copy kernels), and the
// wall-clock heuristics behind the choice; every one the pipeline has is
// here.
//
// MXEC_PIPE_COPY (knobs.hpp): sdma; waves (every host batch); auto (the
// default) -- SDMA while it runs at its normal rate, CU-wave copies while
// it does not (open / judge below).  Measured (profiles/r4/get_stall/,
// e2e_get_modes/): in a healthy process SDMA is the faster engine
// (RS-only GET 0.101 s against 0.119 by waves at 128 objects; the PUT
// with digests 0.218 against 0.264, copy waves beside the SHA-256 chains
// slowing the chains), but after heavy HBM churn SDMA copies collapsed
// for seconds to ~7 GB/s ([0.33, 0.92, 0.33, 0.92, 0.27] s verified GETs
// against 0.263 by waves).
#pragma once

#include <atomic>
#include <chrono>
#include <vector>

#include "runtime.hpp"

namespace mxec {

class CopyWatch {
public:
    // calls: the hub's count of calls in flight on the device.
    CopyWatch(Device& d, hipStream_t h2d, hipStream_t d2h, const std::atomic<int>& calls)
        : d_(d), h2d_(h2d), d2h_(d2h), calls_(calls) {}
    CopyWatch(const CopyWatch&) = delete;
    CopyWatch& operator=(const CopyWatch&) = delete;
    ~CopyWatch() {
        for (auto e : events_) (void)hipEventDestroy(e);
    }

    static int64_t now_ns() {
        return std::chrono::duration_cast<std::chrono::nanoseconds>(
                   std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    bool shared_now() const { return calls_.load() > 1; }
    bool auto_mode() const { return d_.kn && d_.kn->pipe_copy == 2; }
    // This call's copies of mxec_host_alloc memory go by waves.
    bool up_by_waves() const { return up_waves_; }
    bool down_by_waves() const { return down_waves_; }

    // Start of a call: the mode, and under auto the device's holds.
    void start_call() {
        const int mode = d_.kn ? d_.kn->pipe_copy : 0;
        const int64_t now = now_ns();
        up_waves_ = mode == 1 || (mode == 2 && now < d_.waves_up_until_ns.load());
        down_waves_ = mode == 1 || (mode == 2 && now < d_.waves_down_until_ns.load());
    }
    // End of a call: judge what is left (its copies are done), for the
    // device's next calls.
    int end_call() {
        up_.a = down_.a = nullptr;
        up_.on = down_.on = false;
        while (!done_.empty()) MXEC_TRY(judge());
        return MXEC_OK;
    }

    // Copy engine under MXEC_PIPE_COPY=auto: SDMA, watched.  The uploads of
    // each piece (or group) of a wave are bracketed by timing events on the
    // upload stream (open_up / close_up).  The host never waits for a
    // bracket (pacing the enqueue loop two brackets deep held back the group
    // form's downloads: RS-only PUT at 128 objects 0.188 s against 0.112):
    // brackets are judged when the host finds them complete, at the latest
    // when the call has synchronised (end_call).  A bracket of at least
    // kMinBytes (16 MiB) of direct DMAs (no staging ring) that ran
    // below MXEC_PIPE_SDMA_FLOOR GB/s (default 20; healthy 1-4 MiB copies run
    // 33-43, the collapse seen after heavy HBM churn ran ~7) switches the
    // rest of the call's uploads of mxec_host_alloc memory (if any are still
    // to be issued) and the device's for the next kWavesHoldMs to the wave
    // kernels; a download bracket (RS-only GET, below) does the same for
    // downloads.  A slow-down lasts ~3.5 s after 60 GB of HBM is freed
    // (profiles/r5/copy_engine/slow_duration_after_60GB_free_r5m.jsonl).
    //
    // A bracket opens before its copies are queued, but its start event is
    // recorded only after its first SDMA copy (count), which it does not
    // time: an event recorded on an idle copy stream completes at once, and
    // the bracket would then time the host queueing the first copy too
    // (ADVICE r5).
    void open_up() {
        if (watching(false) && !up_.on) up_ = Open{true};
    }
    // After the bracket's copies are issued (HostCopy::issue_up done).
    int close_up() { return close(up_, false); }
    // Downloads (an RS-only GET's rebuilt shards, rebuild_list): the bracket
    // opens after the d2h stream's wait for the rebuild, so it times the
    // copies alone.  The PUT's parity downloads are not bracketed: in the
    // seconds after a large HBM free, timing events among the
    // PUT-with-digests pieces' downloads slowed that call by 63 % (0.336 s
    // against 0.206 at 128 objects,
    // profiles/r5/copy_engine/auto_dwatch_churn60_r5l2.jsonl), and its SDMA
    // downloads otherwise beat waves (0.204 s against 0.238 fresh).
    void open_down() {
        if (watching(true) && !down_off_ && !down_.on) down_ = Open{true};
    }
    int close_down() { return close(down_, true); }
    // After an SDMA copy of `bytes` in `copies` DMAs (2D: rows) was queued.
    int count(bool down, uint64_t bytes, uint64_t copies) {
        Open& o = down ? down_ : up_;
        if (!o.on) return MXEC_OK;
        if (!o.a) {
            MXEC_TRY(new_event(&o.a));
            MXEC_HIP(hipEventRecord(o.a, down ? d2h_ : h2d_));
            return MXEC_OK;
        }
        o.bytes += bytes;
        o.copies += copies;
        return MXEC_OK;
    }
    // A copy went through the staging ring (a host memcpy): the open
    // bracket does not measure an SDMA rate.
    void staged(bool down) { (down ? down_ : up_).staged = true; }

    // A host reconstruct wave begins (ended by end_get_wave): a verified
    // wave's downloads are not bracketed.
    void begin_get_wave(bool verified) {
        down_before_ = down_waves_;
        down_off_ = verified;
        up_forced_ = judge_ = redo_ = false;
    }
    // auto: a chain-bound wave verified as one group uploads by waves
    // (one copy launch per piece instead of a DMA per piece of every
    // shard: 128 x 4+2 x 10 MiB 0.240 s against 0.256 by SDMA, 256
    // objects 0.363 against 0.371); an upload-bound wave keeps SDMA
    // uploads (512: 0.590 against 0.679 by waves, whose copies beside
    // the downloads and chains slow both;
    // profiles/r5/copy_engine/verified_uploads_r5z.jsonl), and so does
    // a call that shares the device.  Measured as a lab setting, since
    // removed.  Until the wave ends; only the override is undone then
    // (ADVICE r5).
    void chain_bound_uploads_by_waves() {
        up_before_ = up_waves_;
        up_forced_ = up_waves_ = true;
    }
    // A lone speculating wave's downloads run beside its chains and
    // uploads: by SDMA, unless an earlier call found them slow there
    // (spec_judge) less than kSpecWavesHoldMs ago; by SDMA, the wave is
    // judged when it ends.
    void lone_speculating_wave() {
        if (!auto_mode()) return;
        const bool sdma = !down_waves_;
        if (now_ns() < d_.spec_waves_until_ns.load()) down_waves_ = true;  // restored at the end
        judge_ = sdma && !down_waves_;
    }
    // A verification group's verdicts are in (redo: some object has to be
    // decoded again, so the wave's tail says nothing about its downloads).
    void verdicts_in(bool redo) {
        t_verdict_ = now_ns();
        redo_ = redo_ || redo;
    }
    // Without speculation the last group's rebuilt shards (on the
    // critical path, alone on the link) go down by waves, earlier
    // groups' by SDMA beside the later groups' uploads and chains
    // (wave copies there slow the chains: 0.64 s against 0.59 at 512
    // objects, G = 2).  Speculative downloads run beside the chains,
    // so they keep SDMA.  (A lone call's groups only.)
    void group_downloads(bool last) {
        if (auto_mode()) down_waves_ = down_before_ || last;
    }
    void end_get_wave(bool ok) {
        if (up_forced_) up_waves_ = up_before_;
        if (ok && judge_ && !redo_) spec_judge();
        judge_ = up_forced_ = false;
        down_waves_ = down_before_;
        down_off_ = false;
    }

private:
    static constexpr uint64_t kMinBytes = uint64_t(16) << 20;
    // Only brackets whose DMAs average at least this much are judged: many
    // small copies run near the floor on a healthy SDMA (a 10 MiB chunk's
    // 256 KiB tail piece, 512 copies, read 9 GB/s in a fresh process).
    static constexpr uint64_t kMinCopy = uint64_t(1) << 20;
    // Downloads hold for 1 s: their slow spells follow HBM frees and last
    // about freed bytes / 17 GB/s, so a 2 s hold after a pool-sized free
    // kept an RS-only GET on waves (0.111 s) after SDMA had recovered
    // (0.101; profiles/r5/copy_engine/vg_churn0_r5s.jsonl).
    static constexpr int kWavesHoldMs = 2000, kDownWavesHoldMs = 1000;
    static constexpr int kDownSlowRun = 2;  // slow download brackets in a row for a verdict
    static constexpr int64_t kSpecTailMs = 25, kSpecWavesHoldMs = 2000;
    struct Open {  // the bracket being queued, one per direction
        bool on = false;
        hipEvent_t a = nullptr;
        bool staged = false;
        uint64_t bytes = 0, copies = 0;  // SDMA bytes issued, and the DMAs (2D: rows) that moved them
    };
    struct Bracket {
        hipEvent_t a, b;
        uint64_t bytes, copies;
        bool staged, down;
    };

    // Not while another call shares the copy streams: its copies would land
    // inside this call's brackets.
    bool watching(bool down) const {
        return auto_mode() && d_.kn->pipe_sdma_floor > 0 && !(down ? down_waves_ : up_waves_) && !shared_now();
    }
    int new_event(hipEvent_t* e) {
        MXEC_HIP(hipEventCreate(e));
        events_.push_back(*e);
        return MXEC_OK;
    }
    int close(Open& o, bool down) {
        if (!o.on) return MXEC_OK;
        o.on = false;
        if (!o.a) return MXEC_OK;  // no SDMA copy to time
        hipEvent_t b = nullptr;
        MXEC_TRY(new_event(&b));
        MXEC_HIP(hipEventRecord(b, down ? d2h_ : h2d_));
        done_.push_back(Bracket{o.a, b, o.bytes, o.copies, o.staged, down});
        o.bytes = o.copies = 0;
        o.a = nullptr;
        while (!done_.empty()) {  // the finished ones, oldest first, without waiting
            if (hipEventQuery(done_.front().b) != hipSuccess) {
                (void)hipGetLastError();
                break;
            }
            MXEC_TRY(judge());
        }
        return MXEC_OK;
    }
    int judge() {
        const Bracket k = done_.front();
        done_.erase(done_.begin());
        MXEC_HIP(hipEventSynchronize(k.b));
        float ms = 0;
        MXEC_HIP(hipEventElapsedTime(&ms, k.a, k.b));
        if (k.staged || k.bytes < kMinBytes || k.bytes < k.copies * kMinCopy || ms <= 0) return MXEC_OK;
        const double gbps = double(k.bytes) / (double(ms) * 1e6);
        // A GET's download brackets run at 54-55 GB/s on a healthy box and
        // ~24 in the seconds after a large HBM free (uploads: 33-55 healthy,
        // unaffected by the free), so they are judged against twice the floor.
        const double floor = double(d_.kn ? d_.kn->pipe_sdma_floor : 20) * (k.down ? 2.0 : 1.0);
        const bool slow = gbps < floor;
        const int64_t hold = now_ns() + int64_t(k.down ? kDownWavesHoldMs : kWavesHoldMs) * 1000000;
        if (k.down) {
            // Two slow download brackets in a row make a verdict: an RS-only
            // GET's downloads share the link with its uploads, and a lone
            // bracket under the bar sent healthy calls to waves for a second
            // (0.128 s against 0.101 by SDMA; profiles/r6/final_r6aq/), where
            // a real slow state repeats bracket after bracket (~24 GB/s).
            ++d_.sdma_down_probes;
            d_.sdma_down_last_mbps = uint64_t(gbps * 1e3);
            if (!slow) {
                d_.down_slow_run = 0;
            } else if (!down_waves_ && d_.down_slow_run.fetch_add(1) + 1 >= kDownSlowRun) {
                d_.down_slow_run = 0;
                ++d_.sdma_down_slow_verdicts;
                down_waves_ = true;  // the rest of this call's downloads
                d_.waves_down_until_ns = hold;
            }
        } else {
            ++d_.sdma_probes;
            d_.sdma_last_mbps = uint64_t(gbps * 1e3);
            if (!up_waves_ && slow) {
                ++d_.sdma_slow_verdicts;
                up_waves_ = true;  // the rest of this call's uploads
                d_.waves_up_until_ns = hold;
            }
        }
        return MXEC_OK;
    }
    // A lone speculating wave's speculative downloads go by SDMA: healthy,
    // they keep pace with the chains and the wave ends ~1 ms after its last
    // verdict (128 x 4+2 x 10 MiB: 0.193 s).  But in some processes, and in
    // the seconds after a large HBM free, those SDMA downloads crawl at
    // ~6 GB/s while the chains run and the same GET takes 0.42-0.47 s; by CU
    // waves it takes 0.24 s in either state (and without speculation 0.242;
    // profiles/r6/spec_grid/get_churn_ab_*.jsonl).  Nothing measured ahead of
    // the wave tells the states apart: a 32 MiB D2H copy on the idle link ran
    // at 54-55 GB/s in both, the same copy beside the first piece's upload
    // at 13.4 GB/s in both (get_churn_ab_r6u/r6v), and the pieces' own
    // download brackets during the upload phase run at ~6 GB/s in both.  So
    // the wave is judged after the fact: downloads still running more than
    // kSpecTailMs after the last verdict (healthy ~1 ms, slow ~140) send the
    // device's next lone speculating waves' downloads to waves for
    // kSpecWavesHoldMs, doubled for each slow verdict in a row up to 16 s;
    // the first wave after the hold tries SDMA again (a healthy one ends the
    // run of slow verdicts).
    void spec_judge() {
        if (!t_verdict_) return;
        const int64_t tail_ms = (now_ns() - t_verdict_) / 1000000;
        ++d_.sdma_down_probes;
        if (tail_ms <= kSpecTailMs) {
            d_.spec_slow_run = 0;
            return;
        }
        ++d_.sdma_down_slow_verdicts;
        const int run = std::min(d_.spec_slow_run.fetch_add(1), 3);
        d_.spec_waves_until_ns = now_ns() + (kSpecWavesHoldMs << run) * 1000000;
    }

    Device& d_;
    const hipStream_t h2d_, d2h_;
    const std::atomic<int>& calls_;
    bool up_waves_ = false, down_waves_ = false;
    Open up_, down_;
    std::vector<Bracket> done_;      // closed, not yet judged
    std::vector<hipEvent_t> events_;  // the brackets' timing events, destroyed with the call
    // the current host reconstruct wave (begin_get_wave)
    bool down_off_ = false, down_before_ = false, up_before_ = false, up_forced_ = false;
    bool judge_ = false, redo_ = false;
    int64_t t_verdict_ = 0;
};

}  // namespace mxec
