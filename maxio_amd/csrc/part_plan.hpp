// part_plan.hpp — the arithmetic of the streaming CompleteMultipartUpload
// (storage_multipart.cpp over storage_writer.cpp; complete_multipart_chunked
// filesystem.rs:1147-1310 and complete_multipart_chunked_encrypted :1315-1560):
// where each part lies in the body, how long an encrypted part's file must be,
// and the steps that feed the parts to an encrypted writer in order -- a
// stretch of a plain part to push through the writer's host path, or one
// decrypt launch of at most 16 part frames into the writer's plaintext ring,
// shared by consecutive encrypted parts.  Only integers; nothing is read or
// written.
//
// Host-only (no HIP, no I/O): storage_multipart.cpp calls it, and
// tests/c_manifest/part_plan_check.cpp runs it against a byte-by-byte model
// under -fsanitize=address,undefined.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "frame_plan.hpp"

namespace mxec {

constexpr uint64_t kFeedFrames = kEncFrames;         // part frames per decrypt launch (at most)
constexpr uint64_t kFeedPiece = uint64_t(1) << 20;   // bytes of a plain part per step (one staging piece)

struct PartSpec {
    uint64_t size;  // plaintext bytes (a plain part's file size)
    bool encrypted;
};
struct PartInfo {
    uint64_t body_off, size;
    bool encrypted;
    uint64_t frames;    // encrypted: frame_count(size), frames of 64 KiB counted from 0 in every part
    uint64_t file_len;  // encrypted: the bytes its file must hold, mxec_frames_len(size, 65536)
};

struct PartPlan {
    std::vector<PartInfo> parts;
    uint64_t body_len = 0;
    uint64_t ring_bytes = 0;
    bool ok = false;  // false: a length does not fit in 64 bits, or the ring is too small for a launch
};

// ring_bytes: the plaintext ring the launches write into; it holds the whole
// body or at least one launch's plaintext (kEncRun).
inline PartPlan part_plan(const PartSpec* parts, size_t n, uint64_t ring_bytes) {
    PartPlan p;
    p.ring_bytes = ring_bytes;
    for (size_t i = 0; i < n; ++i) {
        PartInfo pi{p.body_len, parts[i].size, parts[i].encrypted, 0, 0};
        if (pi.encrypted) {
            pi.frames = frame_count(pi.size);
            if (!frame_stream_len(pi.size, &pi.file_len)) return p;
        }
        if (pi.size > UINT64_MAX - p.body_len) return p;
        p.body_len += pi.size;
        p.parts.push_back(pi);
    }
    p.ok = ring_bytes > 0 && (ring_bytes >= p.body_len || ring_bytes >= kEncRun);
    return p;
}

// One part's share of a launch: `frames` frames from first_frame on.
struct FeedJob {
    uint32_t part;
    uint64_t first_frame, frames;
    uint64_t file_off;      // of first_frame in the part's file
    uint64_t stream_bytes;  // to read from there: plain_bytes + 28 per frame
    uint64_t plain_bytes;
    uint64_t ring_off;      // (body offset of its first byte) % ring_bytes
};
struct FeedStep {
    bool launch;  // false: plain bytes [part_off, part_off + len) of `part`, len <= kFeedPiece
    uint32_t part;
    uint64_t part_off, len;
    // launch: jobs in body order, end to end
    uint32_t n_jobs;
    uint64_t frames;  // <= kFeedFrames
    FeedJob jobs[kFeedFrames];
    // The 1 MiB ring stretches (body offset / kEncRun) whose first byte the
    // launch writes: [open_first, open_first + open_count).  Their previous
    // tenants must have been done with before it is queued.
    uint64_t open_first, open_count;
    uint64_t body_off, body_end;  // the body bytes the step covers; enc_runs_due(body, body_off, body_end) is then due
};

// The feed steps in body order, to f(step) -> status; stops at the first
// non-zero status and returns it.  Consecutive encrypted parts share launches:
// a launch is ended only by its 16th frame, by a plain part or by the end.
// Empty parts take no step.
template <class F>
int part_feed(const PartPlan& p, F&& f) {
    FeedStep L{};
    auto flush = [&]() -> int {
        if (L.n_jobs == 0) return 0;
        L.launch = true;
        const FeedJob& a = L.jobs[0];
        const FeedJob& z = L.jobs[L.n_jobs - 1];
        L.body_off = p.parts[a.part].body_off + a.first_frame * kFramePlain;
        L.body_end = p.parts[z.part].body_off + z.first_frame * kFramePlain + z.plain_bytes;
        L.open_first = L.body_off / kEncRun + (L.body_off % kEncRun ? 1 : 0);
        const uint64_t last = (L.body_end - 1) / kEncRun;  // body_end > body_off: every job has a byte
        L.open_count = last >= L.open_first ? last - L.open_first + 1 : 0;
        const int rc = f(static_cast<const FeedStep&>(L));
        L = FeedStep{};
        return rc;
    };
    for (size_t i = 0; i < p.parts.size(); ++i) {
        const PartInfo& pi = p.parts[i];
        if (!pi.encrypted) {
            if (pi.size == 0) continue;
            if (const int rc = flush()) return rc;
            for (uint64_t off = 0; off < pi.size; off += kFeedPiece) {
                FeedStep s{};
                s.part = uint32_t(i);
                s.part_off = off;
                s.len = pi.size - off < kFeedPiece ? pi.size - off : kFeedPiece;
                s.body_off = pi.body_off + off;
                s.body_end = s.body_off + s.len;
                if (const int rc = f(static_cast<const FeedStep&>(s))) return rc;
            }
            continue;
        }
        for (uint64_t f0 = 0; f0 < pi.frames;) {
            const uint64_t room = kFeedFrames - L.frames, left = pi.frames - f0;
            FeedJob j{};
            j.part = uint32_t(i);
            j.first_frame = f0;
            j.frames = left < room ? left : room;
            j.file_off = frame_stream_off(f0);
            const uint64_t rest = pi.size - f0 * kFramePlain;
            j.plain_bytes = rest < j.frames * kFramePlain ? rest : j.frames * kFramePlain;
            j.stream_bytes = j.plain_bytes + kFrameExtra * j.frames;
            j.ring_off = (pi.body_off + f0 * kFramePlain) % p.ring_bytes;
            L.jobs[L.n_jobs++] = j;
            L.frames += j.frames;
            f0 += j.frames;
            if (L.frames == kFeedFrames)
                if (const int rc = flush()) return rc;
        }
    }
    return flush();
}

}  // namespace mxec
