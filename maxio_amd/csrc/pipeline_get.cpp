// pipeline_get.cpp -- end-to-end host-memory batch reconstruct (the GET path
// as MaxIO sees it: the shards read from the drives in host memory, the
// missing ones rebuilt into host memory, the present ones verified against
// their digests on the way), spread over every device of the context
// (pipeline.hpp).
#include <memory>

#include "pipeline.hpp"

namespace mxec {
namespace {

// One object of a host reconstruct batch (mxec_reconstruct_batch_host).
struct RecObj {
    int k, m;
    uint64_t S;
    uint8_t* const* shards;          // k + m host buffers (present: read; missing: rebuilt into)
    const uint64_t* len;             // k + m, clamped to S
    uint8_t* present;                // k + m, in/out
    const uint8_t (*expected)[32];   // k + m digests, or null (no verification)
    int32_t* status;                 // out: MXEC_OK or MXEC_E_TOO_FEW_SHARDS_PRESENT
    uint64_t pool_off = 0;
    uint64_t slot() const { return rup(S, kAlign); }
    uint64_t bytes() const { return uint64_t(k + m) * slot(); }
    // Its share of a wave's descriptor tables: pointer / length /
    // digest-index tables, the SHA tables and one 16-byte record per tile of
    // the grouped launch (tiles >= 8 KiB).
    uint64_t desc_bytes() const { return uint64_t(k + m) * 96 + 512 + (S / 8192 + 2) * 32; }
};

class GetCall : PipeCall {
public:
    GetCall(Device& d, PipeHub& h, PipeLane& l) : PipeCall(d, h, l, 0) {}
    int run(std::vector<RecObj>& objs, bool data_only) {
        return run_waves(objs, [&](size_t o0, size_t o1) { return rec_wave(objs, o0, o1, data_only); });
    }

private:
    // One wave of a host reconstruct batch (try_reconstruct_data_chunk,
    // chunk_reader.rs:157-226, per object).
    //
    // Verified waves (expected digests given) run piece-major when their
    // messages fit the lag quad form: piece p of every present shard goes up
    // and is hashed with the chains carried in device state slots, so every
    // chain starts after the first piece (verify_enqueue), and -- with
    // MXEC_GET_SPECULATE (default) -- piece p of every missing shard is
    // decoded from the first k present shards as soon as piece p is up, on
    // the assumption that they verify, and goes down at once (spec_piece).
    // The verdict then only confirms: an object whose shards all verified is
    // done; one with a mismatch is decoded again with the corrected mask and
    // its shards overwritten (a mismatch is an erasure, :176-196); one left
    // short of k shards fails with MXEC_E_TOO_FEW_SHARDS_PRESENT -- its
    // present shards untouched, its missing shards' buffers undefined (the
    // reference returns Err and no data, :203-206).  Without speculation the
    // rebuild waits for the verdict (nothing is written to a failing
    // object's buffers), and a large wave runs as a few verification groups
    // (verify_cuts) so that group j's rebuild and download overlap group
    // j + 1's upload and chains; with it the downloads already overlap
    // everything and the wave is one group.
    //
    // Other waves: the present shards go up group by group (coalesced,
    // direct from pinned memory), are verified by one SHA-256 launch once
    // all are up when digests are given, each group is rebuilt (one grouped
    // launch, run_rs_mixed) as soon as it is up (and verified), and its
    // rebuilt shards go down while later groups still upload.
    int rec_wave(std::vector<RecObj>& objs, size_t o0, size_t o1, bool data_only) {
        PTRACE(start(h2d_));
        uint64_t msgs = 0;
        bool verify = false;
        for (size_t o = o0; o < o1; ++o) {
            msgs += uint64_t(objs[o].k + objs[o].m);
            verify = verify || objs[o].expected;
        }
        // Expected digests of the wave (message order) after room for the
        // verdict flags, on the device.
        const uint64_t fo = rup(msgs, 256);
        uint8_t* ok = nullptr;
        uint8_t* exp = nullptr;
        if (verify) {
            MXEC_TRY(scratch_.grow(fo + msgs * 32));
            ok = static_cast<uint8_t*>(scratch_.p);
            exp = ok + fo;
        }
        watch_.begin_get_wave(verify);
        uint64_t vmsgs = 0;  // present shards to verify
        uint64_t up_bytes = 0, longest_msg = 0;
        for (size_t o = o0; o < o1; ++o)
            for (int i = 0; i < objs[o].k + objs[o].m; ++i)
                if (objs[o].present[i]) {
                    up_bytes += objs[o].len[i];
                    if (!objs[o].expected) continue;
                    ++vmsgs;
                    longest_msg = std::max(longest_msg, objs[o].len[i]);
                }
        const uint64_t P = piece_bytes(up_bytes, longest_msg);
        if (verify && P && vmsgs && vmsgs <= lag_capacity()) {
            const bool shared = watch_.shared_now();
            const bool spec = !d_.kn || d_.kn->get_speculate;
            uint64_t down_bytes = 0;
            for (size_t o = o0; o < o1; ++o)
                for (int i = 0; i < objs[o].k + objs[o].m; ++i) down_bytes += objs[o].present[i] ? 0 : objs[o].len[i];
            // One group when speculating (the downloads overlap the chains
            // already) or when another call shares the device (one compute
            // stream each: a second group's chains would queue behind the
            // first's on it).
            const std::vector<size_t> cut = verify_cuts(objs, o0, o1, up_bytes, longest_msg, down_bytes, spec || shared);
            MXEC_TRY(state_.grow(msgs * 32));
            MXEC_TRY(flags_.grow(msgs));
            std::vector<uint64_t> mbase(cut.size(), 0);
            for (size_t j = 1; j < cut.size(); ++j) {
                mbase[j] = mbase[j - 1];
                for (size_t o = cut[j - 1]; o < cut[j]; ++o) mbase[j] += uint64_t(objs[o].k + objs[o].m);
            }
            const size_t G = cut.size() - 1;
            // A chain-bound wave verified as one group, alone on the device.
            if (watch_.auto_mode() && G == 1 && piece_ramp_ && !shared) watch_.chain_bound_uploads_by_waves();
            if (spec && !shared) watch_.lone_speculating_wave();
            std::vector<hipEvent_t> verdict(G, nullptr);
            auto enqueue = [&](size_t j) {
                return verify_enqueue(objs, cut[j], cut[j + 1], ok, exp, mbase[j], P, cs_[(cs_idx_ + int(j)) & 1],
                                      &verdict[j], spec, data_only);
            };
            MXEC_TRY(enqueue(0));
            for (size_t j = 0; j < G; ++j) {
                if (j + 1 < G) MXEC_TRY(enqueue(j + 1));
                std::vector<size_t> changed;
                MXEC_TRY(verify_collect(objs, cut[j], cut[j + 1], mbase[j], verdict[j], &changed));
                PTRACE(now("verified"));
                watch_.verdicts_in(!changed.empty());
                if (spec) {
                    MXEC_TRY(confirm(objs, cut[j], cut[j + 1], changed, data_only));
                    // The objects with a mismatch, decoded again with their
                    // verified masks on the D2H stream: behind the
                    // speculative downloads, which read the slots this
                    // decode rewrites.
                    if (!changed.empty()) {
                        d_.spec_redos += changed.size();
                        MXEC_TRY(rebuild_list(objs, changed, d2h_, nullptr, data_only));
                    }
                } else {
                    if (!shared) watch_.group_downloads(j + 1 == G);
                    for (const auto& q : object_groups(objs, cut[j], cut[j + 1]))
                        MXEC_TRY(rebuild_range(objs, q.first, q.second, cs_[(cs_idx_ + int(j)) & 1], nullptr, data_only));
                }
            }
            d_.verify_groups += G;
            d_.verify_waves += 1;
        } else {
            const auto groups = object_groups(objs, o0, o1);
            hipStream_t cs = cs_[cs_idx_];
            std::vector<hipEvent_t> up;  // per group: its upload is done
            MXEC_TRY(upload_and_verify(objs, o0, o1, groups, ok, exp, verify, cs, &up));
            // Per group, rebuild once it is up (without verification, as soon
            // as it is up), then its shards down.
            for (size_t q = 0; q < groups.size(); ++q)
                MXEC_TRY(rebuild_range(objs, groups[q].first, groups[q].second, cs, verify ? nullptr : up[q], data_only));
        }
        MXEC_TRY(copy_.issue_down());
        PTRACE(mark("d2h", d2h_));
        PTRACE(now("down_queued"));
        const int frc = copy_.flush();
        PTRACE(report("rec_wave"));
        watch_.end_get_wave(frc == MXEC_OK);
        return frc;
    }

    // Workgroups of a speculative piece decode: four per CU.  It runs beside
    // the wave's SHA-256 chains; at the RS kernel's default grid (512-1024
    // per CU, 0.13-0.26 M workgroups for a 1 MiB piece of 128 x 4+2) it
    // either slowed the chains (19 -> 35 ms a piece) or was starved by them
    // (a piece's decode + download 42 ms instead of 9), which of the two
    // changing from call to call: 0.19-0.46 s for the same 128-object GET
    // (pipe traces, profiles/r6/spec_grid/).  A piece's decode moves ~0.8 GB
    // in the ~9 ms the link takes to bring the next piece up; at one
    // workgroup per CU the GET ended ~6 ms later than at four
    // (profiles/r6/spec_grid/spec_grid_ab_r6q.jsonl).
    uint32_t spec_blocks() const { return 4u * (d_.n_cus ? uint32_t(d_.n_cus) : 256u); }

    // Objects [o0, o1) of a speculatively rebuilt group whose present masks
    // the verdict left as they were (all but `changed`): their rebuilt
    // shards are already on their way down; status and present flags.
    int confirm(std::vector<RecObj>& objs, size_t o0, size_t o1, const std::vector<size_t>& changed, bool data_only) {
        size_t c = 0;
        for (size_t o = o0; o < o1; ++o) {
            if (c < changed.size() && changed[c] == o) {
                ++c;
                continue;
            }
            // decode_plan's rule (gf256.cpp): k present shards make a plan,
            // and its missing shards are every absent one (data_only: every
            // absent data shard)
            RecObj& h = objs[o];
            int np = 0;
            for (int i = 0; i < h.k + h.m; ++i) np += h.present[i] ? 1 : 0;
            *h.status = np >= h.k ? MXEC_OK : MXEC_E_TOO_FEW_SHARDS_PRESENT;
            if (np >= h.k)
                for (int i = 0; i < h.k + (data_only ? 0 : h.m); ++i) h.present[i] = 1;
        }
        return MXEC_OK;
    }

    // Consecutive objects up to kGroupBytes of present input.
    static std::vector<std::pair<size_t, size_t>> object_groups(const std::vector<RecObj>& objs, size_t o0,
                                                                size_t o1) {
        std::vector<std::pair<size_t, size_t>> groups;
        for (size_t g0 = o0; g0 < o1;) {
            size_t g1 = g0;
            uint64_t in_bytes = 0;
            while (g1 < o1) {
                uint64_t b = 0;
                for (int i = 0; i < objs[g1].k + objs[g1].m; ++i) b += objs[g1].present[i] ? objs[g1].len[i] : 0;
                if (g1 > g0 && in_bytes + b > kGroupBytes) break;
                in_bytes += b;
                ++g1;
            }
            groups.emplace_back(g0, g1);
            g0 = g1;
        }
        return groups;
    }

    // Verification groups of a piece-major reconstruct wave: cut points
    // (first o0, last o1) by upload bytes; MXEC_GET_VGROUPS of them, or (0,
    // the default) the count the model below picks per wave.  Group j + 1's
    // pieces go up and hash while group j's verdicts come back and its
    // rebuilt shards go down, so only the last group's download follows the
    // last verdict.  Measured at 512 x 4+2 x 10 MiB with SDMA downloads
    // (profiles/r5/get_groups/vgroups_*_r5q.jsonl): one group 0.634 s, two
    // 0.588, three 0.584, four 0.618; with every group's download by waves
    // no count gained (0.637-0.690: wave copies beside the later groups'
    // SHA-256 chains slow the chains).  Round 5's first measurement (one
    // 0.655, two 0.818) predates the one-copy expected-digest upload.
    // `one`: one group unless MXEC_GET_VGROUPS forces a count (rec_wave).
    std::vector<size_t> verify_cuts(const std::vector<RecObj>& objs, size_t o0, size_t o1, uint64_t up_bytes,
                                    uint64_t longest, uint64_t down_bytes, bool one) const {
        int G = d_.kn ? int(d_.kn->get_vgroups) : 1;
        if (G == 0 && one) G = 1;
        if (G == 0) {
            // Per wave: the G that minimises max(T, (G-1)/G T + C) + D/G --
            // the upload T (~50 GB/s), the chain C of the longest message,
            // the rebuilt shards' download D (~55 GB/s), of which only the
            // last group's is on the critical path.  512 x 4+2 x 10 MiB: 2
            // (0.588 s against 0.634 for one group, with SDMA downloads);
            // 128: 1 (the chain outlasts the upload).
            const double T = double(up_bytes) / 50e9, D = double(down_bytes) / 55e9;
            const double C = double(longest / 64) * kShaLagUsPerBlock * 1e-6;
            double best = 0;
            for (int g = 1; g <= 4; ++g) {
                const double t = std::max(T, (g - 1) * T / g + C) + D / g + 0.005 * (g - 1);
                if (g == 1 || t < best) {
                    best = t;
                    G = g;
                }
            }
        }
        std::vector<size_t> cut{o0};
        const size_t n = o1 - o0;
        if (G > 1 && n >= size_t(G)) {
            uint64_t acc = 0;
            int next = 1;
            for (size_t o = o0; o < o1 && next < G; ++o) {
                for (int i = 0; i < objs[o].k + objs[o].m; ++i) acc += objs[o].present[i] ? objs[o].len[i] : 0;
                if (double(acc) >= double(up_bytes) * next / G && o + 1 < o1) {
                    cut.push_back(o + 1);
                    ++next;
                }
            }
        }
        cut.push_back(o1);
        return cut;
    }

    // The expected digests of objects [o0, o1) (message order from message
    // mb) up in one copy: one per object went through the four-buffer
    // staging ring, so every fourth object waited for the upload stream to
    // reach the copy three objects back (the host enqueue crawled beside the
    // GPU, and so did the watch's bracket around it).
    int upload_expected(const std::vector<RecObj>& objs, size_t o0, size_t o1, uint8_t* exp, uint64_t mb) {
        uint64_t gm = 0;
        bool any = false;
        for (size_t o = o0; o < o1; ++o) {
            gm += uint64_t(objs[o].k + objs[o].m);
            any = any || objs[o].expected;
        }
        if (!any || !gm) return MXEC_OK;
        exp_host_.assign(gm * 32, 0);
        uint64_t g = 0;
        for (size_t o = o0; o < o1; ++o) {
            const RecObj& h = objs[o];
            if (h.expected) std::memcpy(&exp_host_[g * 32], &h.expected[0][0], uint64_t(h.k + h.m) * 32);
            g += uint64_t(h.k + h.m);
        }
        MXEC_TRY(copy_.flush_up());
        return copy_.upload(exp + mb * 32, exp_host_.data(), gm * 32);
    }
    std::vector<uint8_t> exp_host_;  // staging source of upload_expected (consumed by upload's ring copy)

    // The decode of bytes [off, off + pw) of objects `which`: each object's
    // missing shards from its decode plan (plans[t]; none when it is short
    // of k shards or ends before off), in one grouped launch on s
    // (decode_step over the pool's slots; blocks: its workgroup cap, 0 = the
    // default grid).  A whole-shard rebuild is off 0, pw unbounded.
    int decode_piece(const std::vector<RecObj>& objs, const std::vector<size_t>& which, uint64_t off, uint64_t pw,
                     bool data_only, hipStream_t s, uint32_t blocks,
                     std::vector<std::shared_ptr<const DecodePlan>>& plans) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        std::vector<DecodeItem> items;
        items.reserve(which.size());
        for (size_t o : which) {
            const RecObj& h = objs[o];
            items.push_back(DecodeItem{h.k, h.m, h.S, h.len, h.present, nullptr, base + h.pool_off, h.slot()});
        }
        return decode_step(d_, slot_, s, std::move(items), data_only, plans, off, pw, &arena_, blocks);
    }

    // Objects `which` of a wave, their present shards up (or verified):
    // rebuild each object's missing shards from its decode plan (one grouped
    // launch, run_rs_mixed, on cs after `up` if given), then send them down
    // to the caller's buffers and mark them present.  An object short of k
    // shards gets MXEC_E_TOO_FEW_SHARDS_PRESENT and none of its buffers is
    // written here.
    int rebuild_range(std::vector<RecObj>& objs, size_t q0, size_t q1, hipStream_t cs, hipEvent_t up, bool data_only) {
        std::vector<size_t> which(q1 - q0);
        for (size_t o = q0; o < q1; ++o) which[o - q0] = o;
        return rebuild_list(objs, which, cs, up, data_only);
    }
    int rebuild_list(std::vector<RecObj>& objs, const std::vector<size_t>& which, hipStream_t cs, hipEvent_t up,
                     bool data_only) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        if (cs == d2h_) MXEC_TRY(copy_.issue_down());  // wave copy blocks queued for d2h go before this launch
        if (up) MXEC_HIP(hipStreamWaitEvent(cs, up, 0));
        const size_t n = which.size();
        std::vector<std::shared_ptr<const DecodePlan>> plans;
        MXEC_TRY(decode_piece(objs, which, 0, ~uint64_t(0), data_only, cs, 0, plans));
        PTRACE(mark("rs", cs));
        PTRACE(now("rs_queued"));
        MXEC_TRY(copy_.issue_down());
        if (cs != d2h_) {
            hipEvent_t rs_done;
            MXEC_TRY(copy_.new_event(&rs_done));
            MXEC_HIP(hipEventRecord(rs_done, cs));
            MXEC_HIP(hipStreamWaitEvent(d2h_, rs_done, 0));
        }
        watch_.open_down();
        for (size_t t = 0; t < n; ++t) {
            RecObj& h = objs[which[t]];
            const auto& p = plans[t];
            *h.status = p ? MXEC_OK : MXEC_E_TOO_FEW_SHARDS_PRESENT;
            if (!p) continue;
            for (int e : p->missing) {
                MXEC_TRY(copy_.queue_down(h.shards[e], base + h.pool_off + uint64_t(e) * h.slot(), h.len[e]));
                if (h.len[e] != h.slot()) MXEC_TRY(copy_.flush_down());
                h.present[e] = 1;
            }
        }
        MXEC_TRY(copy_.flush_down());
        return watch_.close_down();
    }

    // Speculative rebuild of piece [off, off + pw) of objects `which`
    // (MXEC_GET_SPECULATE): once the piece of every present shard is up
    // (`up`), the same piece of each object's missing shards is decoded from
    // its first k present shards -- RS is bytewise, so a piece of the output
    // comes from the same piece of the inputs, as in the PUT's piece-major
    // encode -- and goes down to the caller's buffers.  Launch and downloads
    // both on the D2H stream, so the downloads follow the decode in order.
    // An object short of k present shards is skipped (it fails anyway).
    int spec_piece(std::vector<RecObj>& objs, const std::vector<size_t>& which, uint64_t off, uint64_t pw,
                   hipEvent_t up, bool data_only) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        const size_t n = which.size();
        std::vector<std::shared_ptr<const DecodePlan>> plans;
        MXEC_TRY(copy_.flush_down());
        MXEC_TRY(copy_.issue_down());  // wave copy blocks queued earlier go before the wait
        MXEC_HIP(hipStreamWaitEvent(d2h_, up, 0));
        MXEC_TRY(decode_piece(objs, which, off, pw, data_only, d2h_, spec_blocks(), plans));
        bool any = false;
        for (size_t t = 0; t < n; ++t) {
            if (!plans[t]) continue;
            const RecObj& h = objs[which[t]];
            for (int e : plans[t]->missing) {
                const uint64_t L = h.len[e];
                if (off >= L) continue;
                MXEC_TRY(copy_.queue_down(h.shards[e] + off, base + h.pool_off + uint64_t(e) * h.slot() + off,
                                          std::min(pw, L - off)));
                any = true;
            }
        }
        MXEC_TRY(copy_.flush_down());
        PTRACE(mark("sdown", d2h_));
        if (any) ++d_.spec_pieces;
        return MXEC_OK;
    }

    // Piece-major upload of every present shard of objects [o0, o1) (and the
    // expected digests), each piece of the shards to verify hashed on cs as
    // soon as it is up with the chains carried in device state slots
    // (run_sha_pieces, slot = message index in the wave starting at mb,
    // verdict ok[slot]); after the last piece the verdicts are copied back
    // and *verdict recorded.  Returns without waiting.
    // P: the wave's piece size (piece_bytes over the whole wave: a group's
    // copies are as large as the wave's, whatever its share of the upload).
    // Above 1 MiB the same piece of an object's adjacent present shards goes
    // up as one 2D copy, as in the PUT's upload-bound waves.
    // spec: each piece's missing shards are also decoded and sent down as
    // soon as the piece is up (spec_piece).
    int verify_enqueue(std::vector<RecObj>& objs, size_t o0, size_t o1, uint8_t* ok, uint8_t* exp, uint64_t mb,
                       uint64_t P, hipStream_t cs, hipEvent_t* verdict, bool spec, bool data_only) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        uint32_t* state = static_cast<uint32_t*>(state_.p);
        uint64_t longest = 0, gm = 0;
        for (size_t o = o0; o < o1; ++o) {
            gm += uint64_t(objs[o].k + objs[o].m);
            for (int i = 0; i < objs[o].k + objs[o].m; ++i)
                if (objs[o].present[i]) longest = std::max(longest, objs[o].len[i]);
        }
        PieceGrid grid(P, piece_ramp_);
        std::vector<size_t> group(spec ? o1 - o0 : 0);  // the objects spec_piece decodes
        for (size_t t = 0; t < group.size(); ++t) group[t] = o0 + t;
        MXEC_TRY(upload_expected(objs, o0, o1, exp, mb));
        HostCopy::Pieces2D twod(copy_, !watch_.up_by_waves() && P > (uint64_t(1) << 20));
        for (uint64_t pc = 0; pc < grid.count(longest); ++pc) {
            widen_if_shared(grid, pc);
            // the ramp's small pieces are not timed: their many small copies
            // run near the floor on a healthy SDMA (a false verdict sent the
            // default line's PUT with digests to waves, 0.316 s)
            if (grid.width(pc) == grid.P) watch_.open_up();
            const uint64_t off = grid.start(pc), pw = grid.width(pc);
            uint64_t g = mb;
            std::vector<const uint8_t*> sp;
            std::vector<uint64_t> sl, st;
            std::vector<uint32_t> ss;
            for (size_t o = o0; o < o1; ++o) {
                const RecObj& h = objs[o];
                for (int i = 0; i < h.k + h.m; ++i, ++g) {
                    if (!h.present[i]) continue;
                    const uint64_t L = h.len[i];
                    uint8_t* dev = base + h.pool_off + uint64_t(i) * h.slot();
                    if (off < L) MXEC_TRY(copy_.queue_up(dev + off, h.shards[i] + off, std::min(pw, L - off)));
                    if (!h.expected || (off >= L && !(pc == 0 && L == 0))) continue;
                    const uint64_t len = L > off ? std::min(pw, L - off) : 0;
                    sp.push_back(dev + off);
                    sl.push_back(len);
                    st.push_back(off + len == L ? L : kShaNotFinal);
                    ss.push_back(uint32_t(g));
                }
            }
            MXEC_TRY(copy_.flush_up());
            hipEvent_t up;
            MXEC_TRY(copy_.new_event(&up));
            MXEC_TRY(copy_.issue_up());
            MXEC_HIP(hipEventRecord(up, h2d_));
            MXEC_TRY(watch_.close_up());
            PTRACE(mark("up", h2d_));
            MXEC_HIP(hipStreamWaitEvent(cs, up, 0));
            if (!sp.empty())
                MXEC_TRY(run_sha_pieces(d_, slot_, cs, sp, sl, ss, st, state, pc > 0, nullptr, &arena_, exp, ok));
            PTRACE(mark("sha", cs));
            if (spec) MXEC_TRY(spec_piece(objs, group, off, pw, up, data_only));
            MXEC_TRY(copy_.pace(up));
        }
        copy_.end_pacing();
        PTRACE(now("pieces_queued"));
        MXEC_HIP(hipMemcpyAsync(static_cast<uint8_t*>(flags_.p) + mb, ok + mb, gm, hipMemcpyDeviceToHost, cs));
        MXEC_TRY(copy_.new_event(verdict));
        MXEC_HIP(hipEventRecord(*verdict, cs));
        return MXEC_OK;
    }

    // Waits for objects [o0, o1)'s verdicts (verify_enqueue): a mismatch
    // becomes an erasure (chunk_reader.rs:176-196).
    // The objects whose masks changed go to *changed (ascending).
    int verify_collect(std::vector<RecObj>& objs, size_t o0, size_t o1, uint64_t mb, hipEvent_t verdict,
                       std::vector<size_t>* changed) {
        MXEC_HIP(hipEventSynchronize(verdict));
        const auto* okh = static_cast<const uint8_t*>(flags_.p);
        uint64_t g = mb;
        for (size_t o = o0; o < o1; ++o) {
            RecObj& h = objs[o];
            bool c = false;
            for (int i = 0; i < h.k + h.m; ++i, ++g)
                if (h.expected && h.present[i] && !okh[g]) {
                    h.present[i] = 0;
                    c = true;
                }
            if (c) changed->push_back(o);
        }
        return MXEC_OK;
    }

    // Phase 1: every upload, one event per group; phase 2 (verification
    // only): one launch over every present shard of the objects that carry
    // digests once all are up, verdicts read back.
    int upload_and_verify(std::vector<RecObj>& objs, size_t o0, size_t o1,
                          const std::vector<std::pair<size_t, size_t>>& groups, uint8_t* ok, uint8_t* exp, bool verify,
                          hipStream_t cs, std::vector<hipEvent_t>* up_out) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        std::vector<hipEvent_t>& up = *up_out;
        up.assign(groups.size(), nullptr);
        if (verify) MXEC_TRY(upload_expected(objs, o0, o1, exp, 0));
        uint64_t g = 0;
        for (size_t q = 0; q < groups.size(); ++q) {
            watch_.open_up();
            for (size_t o = groups[q].first; o < groups[q].second; ++o) {
                const RecObj& h = objs[o];
                for (int i = 0; i < h.k + h.m; ++i) {
                    if (!h.present[i]) continue;
                    MXEC_TRY(copy_.queue_up(base + h.pool_off + uint64_t(i) * h.slot(), h.shards[i], h.len[i]));
                    if (h.len[i] != h.slot()) MXEC_TRY(copy_.flush_up());
                }
                MXEC_TRY(copy_.flush_up());
                g += uint64_t(h.k + h.m);
            }
            MXEC_TRY(copy_.flush_up());
            MXEC_TRY(copy_.new_event(&up[q]));
            MXEC_TRY(copy_.issue_up());
            MXEC_HIP(hipEventRecord(up[q], h2d_));
            MXEC_TRY(watch_.close_up());
            MXEC_TRY(copy_.pace(up[q]));
        }
        copy_.end_pacing();
        if (verify) {
            std::vector<const uint8_t*> sp;
            std::vector<uint64_t> sl, idx;
            std::vector<std::pair<size_t, int>> who;  // message -> (object, shard)
            g = 0;
            for (size_t o = o0; o < o1; ++o) {
                const RecObj& h = objs[o];
                for (int i = 0; i < h.k + h.m; ++i, ++g) {
                    if (!h.expected || !h.present[i]) continue;
                    sp.push_back(base + h.pool_off + uint64_t(i) * h.slot());
                    sl.push_back(h.len[i]);
                    idx.push_back(g);
                    who.emplace_back(o, i);
                }
            }
            MXEC_HIP(hipStreamWaitEvent(cs, up.back(), 0));
            if (!sp.empty()) {
                MXEC_TRY(run_sha(d_, slot_, cs, sp, sl, nullptr, exp, ok, &idx, &arena_));
                MXEC_TRY(flags_.grow(sp.size()));
                MXEC_HIP(hipMemcpyAsync(flags_.p, ok, sp.size(), hipMemcpyDeviceToHost, cs));
                MXEC_TRY(copy_.sync_point(cs));  // not the stream: another call's work may follow on it
                const auto* okh = static_cast<const uint8_t*>(flags_.p);
                for (size_t t = 0; t < who.size(); ++t)
                    if (!okh[t]) objs[who[t].first].present[who[t].second] = 0;
            }
        }
        return MXEC_OK;
    }
};

}  // namespace
}  // namespace mxec

using namespace mxec;

extern "C" int mxec_reconstruct_batch_host(mxec_ctx* ctx, const mxec_object* objs, uint64_t n_obj,
                                           uint8_t* const* shards, const uint64_t* shard_len, uint8_t* present,
                                           const uint8_t (*expected_sha256)[32], uint32_t flags,
                                           int32_t* status_out) {
    try {
        if (n_obj == 0) return MXEC_OK;
        if (!ctx || !objs || !shards || !present) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const size_t D = ctx->c.devs.size();
        if (!D) return set_error(MXEC_E_NO_DEVICE, "context has no device");
        uint64_t sum = 0;
        for (uint64_t o = 0; o < n_obj; ++o) {
            MXEC_TRY(reconstruct_shape(objs[o].k, objs[o].m, objs[o].shard_size));
            sum += uint64_t(objs[o].k + objs[o].m);
        }
        // Every shard pointer is needed: present ones are read, missing ones
        // are where the rebuilt bytes go.
        for (uint64_t g = 0; g < sum; ++g)
            if (!shards[g]) return set_error(MXEC_E_INVALID_ARG, "null shard pointer " + std::to_string(g));
        std::vector<uint64_t> len(size_t(sum), 0);
        std::vector<int32_t> st(size_t(n_obj), MXEC_OK);
        std::vector<uint64_t> obj_bytes(size_t(n_obj), 0);
        std::vector<RecObj> all;
        all.reserve(size_t(n_obj));
        uint64_t g0 = 0;
        for (uint64_t o = 0; o < n_obj; ++o) {
            const int k = objs[o].k, m = objs[o].m;
            const uint64_t S = objs[o].shard_size;
            for (int i = 0; i < k + m; ++i) len[g0 + uint64_t(i)] = shard_len ? std::min<uint64_t>(shard_len[g0 + i], S) : S;
            all.push_back(RecObj{k, m, S, shards + g0, &len[g0], present + g0,
                                 expected_sha256 ? expected_sha256 + g0 : nullptr, &st[o]});
            obj_bytes[o] = all.back().bytes();
            g0 += uint64_t(k + m);
        }
        std::vector<const void*> first(size_t(n_obj), nullptr);
        for (uint64_t o = 0; o < n_obj; ++o)
            for (int i = 0; i < all[o].k + all[o].m && !first[o]; ++i)
                if (all[o].present[i]) first[o] = all[o].shards[i];
        const std::vector<uint32_t> owner = deal_batch(ctx->c, obj_bytes, first);
        std::vector<std::vector<RecObj>> per(D);
        for (uint64_t o = 0; o < n_obj; ++o) per[owner[o]].push_back(all[o]);
        const bool data_only = (flags & MXEC_F_DATA_ONLY) != 0;
        MXEC_TRY(for_each_device(ctx->c, per, [&](Device& dev, PipeHub& hub, PipeLane& lane, std::vector<RecObj>& mine) {
            return GetCall(dev, hub, lane).run(mine, data_only);
        }));
        return reconstruct_status(objs, n_obj, present, st, status_out);
    } catch (const std::bad_alloc&) {
        return set_error(MXEC_E_OOM, "host allocation failed");
    } catch (const std::exception& e) {
        return set_error(MXEC_E_INVALID_ARG, e.what());
    }
}
