// host_copy.cpp -- the parts of HostCopy that run once per piece or wave (host_copy.hpp).
#include "host_copy.hpp"

namespace mxec {

int HostCopy::sync_point(hipStream_t s) {
    hipEvent_t e;
    MXEC_TRY(new_event(&e));
    MXEC_HIP(hipEventRecord(e, s));
    MXEC_HIP(hipEventSynchronize(e));
    return MXEC_OK;
}

int HostCopy::pace(hipEvent_t up) {
    paced_.emplace_back(up, up_since_pace_);
    up_since_pace_ = 0;
    auto ahead = [&] {  // queued before the newest entry
        uint64_t b = 0;
        for (size_t i = 0; i + 1 < paced_.size(); ++i) b += paced_[i].second;
        return b;
    };
    while (paced_.size() > 1) {
        hipEvent_t e = paced_.front().first;
        const hipError_t q = hipEventQuery(e);
        if (q == hipSuccess) {
            paced_.pop_front();
            continue;
        }
        (void)hipGetLastError();
        if (!watch_.shared_now() || ahead() <= kPaceBytes) break;
        ++d_.pace_waits;
        PTRACE(now("pace"));
        MXEC_HIP(hipEventSynchronize(e));
        PTRACE(now("paced"));
        paced_.pop_front();
    }
    return MXEC_OK;
}

// The block table goes into the arena's page-locked host half, which the
// kernel reads in place (no table upload through the copy engines).
int HostCopy::issue_blocks(std::vector<CopyBlk>& v, bool to_host, hipStream_t s) {
    if (v.empty()) return MXEC_OK;
    const size_t bytes = (v.size() * sizeof(CopyBlk) + 255) & ~size_t(255);
    char* h = nullptr;
    char* d = nullptr;
    MXEC_TRY(arena_.take(bytes, &h, &d));
    std::memcpy(h, v.data(), v.size() * sizeof(CopyBlk));
    MXEC_HIP(launch_copy_blocks(reinterpret_cast<const CopyBlk*>(h), v.size(), to_host, kCopyGrid, s));
    d_.copy_wave_blocks += v.size();
    v.clear();
    return MXEC_OK;
}

int HostCopy::drain_next() {
    const int r = out_.next();
    for (size_t i = 0; i < pend_.size(); ++i) {
        if (pend_[i].ring != r) continue;
        MXEC_HIP(hipEventSynchronize(out_.event(r)));
        std::memcpy(pend_[i].dst, out_.ptr(r), pend_[i].len);
        pend_.erase(pend_.begin() + long(i));
        break;
    }
    return MXEC_OK;
}

int HostCopy::flush() {
    MXEC_TRY(issue_down());  // marks what it issues
    if (d2h_mark_) MXEC_HIP(hipEventSynchronize(d2h_mark_));
    for (auto& p : pend_) std::memcpy(p.dst, out_.ptr(p.ring), p.len);
    pend_.clear();
    out_.release_all();
    return MXEC_OK;
}

}  // namespace mxec
