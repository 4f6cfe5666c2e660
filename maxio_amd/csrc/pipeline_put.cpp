// pipeline_put.cpp -- end-to-end host-memory batch encode (the PUT path as
// MaxIO sees it: request bodies in host memory, parity chunks and digests
// back in host memory), spread over every device of the context
// (pipeline.hpp).  Results are bit-identical to mxec_encode.
#include <map>
#include <tuple>

#include "pipeline.hpp"

namespace mxec {
namespace {

struct HostObj {
    int k, m;
    uint64_t S;
    const uint8_t* const* data;
    const uint64_t* dlen;
    uint8_t* const* parity;
    uint8_t (*dig)[32];
    uint64_t pool_off = 0;  // device image: k+m shard slots of rup(S) bytes
    uint64_t slot() const { return rup(S, kAlign); }
    uint64_t bytes() const { return uint64_t(k + m) * slot(); }
    uint64_t desc_bytes() const { return uint64_t(k + m) * 48 + 256; }  // its share of a wave's descriptor tables
};

class PutCall : PipeCall {
public:
    PutCall(Device& d, PipeHub& h, PipeLane& l) : PipeCall(d, h, l, 1) {}
    int run(std::vector<HostObj>& objs) {
        return run_waves(objs, [&](size_t o0, size_t o1) { return wave(objs, o0, o1); });
    }

private:
    // Parity of bytes [off, off + pw) of objects [o0, o1) on s, one launch
    // per (k, m, S) class.  RS is bytewise, so a piece of the parity comes
    // from the same bytes of the data (short data chunks read as zeros past
    // their end); the group form encodes whole shards (off 0, pw unbounded).
    int encode_piece(std::vector<HostObj>& objs, size_t o0, size_t o1, uint64_t off, uint64_t pw, hipStream_t s) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        std::map<std::tuple<int, int, uint64_t>, std::vector<size_t>> classes;
        for (size_t o = o0; o < o1; ++o)
            if (objs[o].S > off) classes[{objs[o].k, objs[o].m, objs[o].S}].push_back(o);
        for (auto& c : classes) {
            const int k = std::get<0>(c.first), m = std::get<1>(c.first);
            const uint64_t S = std::get<2>(c.first), W = std::min(pw, S - off);
            uint32_t coff = 0;
            const size_t n = c.second.size();
            std::vector<const uint8_t*> ins(n * size_t(k));
            std::vector<uint8_t*> outs(n * size_t(m));
            std::vector<uint64_t> lens(n * size_t(k + m), W);
            std::vector<RsObject> ro(n);
            for (size_t t = 0; t < n; ++t) {
                const HostObj& h = objs[c.second[t]];
                uint8_t* ob = base + h.pool_off + off;
                for (int j = 0; j < k; ++j) {
                    ins[t * k + j] = ob + uint64_t(j) * h.slot();
                    const uint64_t L = std::min<uint64_t>(h.dlen[j], S);
                    lens[t * (k + m) + j] = L > off ? std::min(W, L - off) : 0;
                }
                for (int i = 0; i < m; ++i) outs[t * m + i] = ob + uint64_t(k + i) * h.slot();
                ro[t] = RsObject{&ins[t * k], &lens[t * (k + m)], &outs[t * m], &lens[t * (k + m) + k], 0};
            }
            MXEC_TRY(with_stable_coef(
                d_, s, [&] { return encode_coef(d_, k, m, &coff); },
                [&] {
                    for (auto& r : ro) r.coef_off = coff;
                    return run_rs(d_, slot_, s, W, k, m, ro, &arena_);
                }));
        }
        return MXEC_OK;
    }
    // The wave's digests (message order, after sha_done) to the objects that asked for them.
    int digests_down(std::vector<HostObj>& objs, size_t o0, size_t o1, const uint8_t* digests, hipEvent_t sha_done) {
        MXEC_TRY(copy_.issue_down());
        MXEC_HIP(hipStreamWaitEvent(d2h_, sha_done, 0));
        uint64_t msg0 = 0;
        for (size_t o = o0; o < o1; ++o) {
            const HostObj& h = objs[o];
            if (!h.dig) continue;
            MXEC_TRY(copy_.queue_down(reinterpret_cast<uint8_t*>(h.dig), digests + msg0 * 32, uint64_t(h.k + h.m) * 32));
            msg0 += uint64_t(h.k + h.m);
        }
        return copy_.flush_down();
    }

    // Piece-major form of a wave with digests (MXEC_PIPE_PIECE_MB, default 1;
    // 0 = the group form below).  The group form uploads object after object
    // and hashes once all parity exists, so the last-uploaded chunk's chain
    // (163 840 blocks for 10 MiB) starts after the whole upload: 94 + 203 ms
    // for 128 x 4+2 x 10 MiB.  Here piece p (bytes [pP, (p+1)P) of every
    // chunk) goes up, is encoded, hashed -- the chains carried from piece to
    // piece in device state slots (run_sha_pieces) -- and its parity goes
    // down, piece after piece, so every chain starts after the first piece
    // (~9 ms) and the wave ends near one chain's length.  Taken when the
    // wave's messages fit the lag quad form (64 per CU).
    int wave_pieces(std::vector<HostObj>& objs, size_t o0, size_t o1, uint64_t P) {
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        // Chains: every chunk of every object that wants digests, message order.
        struct Chain {
            uint8_t* dev;
            uint64_t len;
        };
        std::vector<Chain> ch;
        uint64_t longest = 0;
        for (size_t o = o0; o < o1; ++o) {
            const HostObj& h = objs[o];
            longest = std::max(longest, h.S);
            if (!h.dig) continue;
            for (int j = 0; j < h.k + h.m; ++j)
                ch.push_back(Chain{base + h.pool_off + uint64_t(j) * h.slot(),
                                   j < h.k ? std::min<uint64_t>(h.dlen[j], h.S) : h.S});
        }
        const uint64_t nm = ch.size();
        MXEC_TRY(scratch_.grow(nm * 64));  // digests [nm][32], then chain states [nm][8] words
        uint8_t* digests = static_cast<uint8_t*>(scratch_.p);
        uint32_t* state = reinterpret_cast<uint32_t*>(digests + nm * 32);
        PieceGrid grid(P, piece_ramp_);
        // RS and the chains on the call's compute stream (PipeHub::use): each
        // piece's RS ahead of its hash, so no piece of this call waits behind
        // another call's chains.
        hipStream_t sha_s = cs_[cs_idx_], rs_s = sha_s;
        hipEvent_t sha_done = nullptr;
        // 2D piece copies for this wave's SDMA copies (queue_up)
        HostCopy::Pieces2D twod(copy_, !watch_.up_by_waves() && P > (uint64_t(1) << 20));
        PTRACE(start(h2d_));
        for (uint64_t pc = 0; pc < grid.count(longest); ++pc) {
            widen_if_shared(grid, pc);
            // No SDMA watch here: in the seconds after a large HBM free the
            // bracket events among the pieces cost the PUT with digests 63 %
            // (0.335 s against 0.206 unwatched at 128 objects,
            // profiles/r5/copy_engine/final_churn60_r5ag.jsonl) while its
            // uploads ran at full rate; its downloads, the direction that
            // slows, stay on SDMA either way (waves cost it 14-18 %).
            const uint64_t off = grid.start(pc), pw = grid.width(pc);
            for (size_t o = o0; o < o1; ++o) {
                const HostObj& h = objs[o];
                for (int j = 0; j < h.k; ++j) {
                    const uint64_t L = std::min<uint64_t>(h.dlen[j], h.S);
                    if (off < L)
                        MXEC_TRY(copy_.queue_up(base + h.pool_off + uint64_t(j) * h.slot() + off, h.data[j] + off,
                                          std::min(pw, L - off)));
                }
            }
            MXEC_TRY(copy_.flush_up());
            hipEvent_t up, rs_done;
            MXEC_TRY(copy_.new_event(&up));
            MXEC_TRY(copy_.new_event(&rs_done));
            MXEC_TRY(copy_.issue_up());
            MXEC_HIP(hipEventRecord(up, h2d_));
            MXEC_TRY(watch_.close_up());
            PTRACE(mark("up", h2d_));
            PTRACE(now("up_queued"));
            MXEC_HIP(hipStreamWaitEvent(rs_s, up, 0));
            MXEC_TRY(encode_piece(objs, o0, o1, off, pw, rs_s));
            MXEC_HIP(hipEventRecord(rs_done, rs_s));
            // This piece of every chain (the hash stream runs the pieces in
            // order, each continuing the chains the previous one left).
            std::vector<const uint8_t*> sp;
            std::vector<uint64_t> sl, st;
            std::vector<uint32_t> ss;
            for (uint64_t q = 0; q < nm; ++q) {
                const Chain& c = ch[q];
                if (off >= c.len && !(pc == 0 && c.len == 0)) continue;  // ended in an earlier piece
                const uint64_t len = c.len > off ? std::min(pw, c.len - off) : 0;
                sp.push_back(c.dev + off);
                sl.push_back(len);
                st.push_back(off + len == c.len ? c.len : kShaNotFinal);
                ss.push_back(uint32_t(q));
            }
            if (!sp.empty()) {
                MXEC_HIP(hipStreamWaitEvent(sha_s, rs_done, 0));
                MXEC_TRY(run_sha_pieces(d_, slot_, sha_s, sp, sl, ss, st, state, pc > 0, digests, &arena_));
                PTRACE(mark("sha", sha_s));
            }
            PTRACE(mark("rs", rs_s));
            // This piece of every parity chunk goes down.
            MXEC_TRY(copy_.issue_down());
            MXEC_HIP(hipStreamWaitEvent(d2h_, rs_done, 0));
            for (size_t o = o0; o < o1; ++o) {
                const HostObj& h = objs[o];
                if (h.S <= off) continue;
                uint8_t* ob = base + h.pool_off + off;
                for (int i = 0; i < h.m; ++i)
                    MXEC_TRY(copy_.queue_down(h.parity[i] + off, ob + uint64_t(h.k + i) * h.slot(), std::min(pw, h.S - off)));
            }
            MXEC_TRY(copy_.flush_down());
            PTRACE(mark("down", d2h_));
            PTRACE(now("piece_queued"));
            MXEC_TRY(copy_.pace(up));
        }
        copy_.end_pacing();
        if (nm) {
            MXEC_TRY(copy_.new_event(&sha_done));
            MXEC_HIP(hipEventRecord(sha_done, sha_s));
            MXEC_TRY(digests_down(objs, o0, o1, digests, sha_done));
        }
        const int frc = copy_.flush();
        PTRACE(report("wave_pieces"));
        return frc;
    }

    // One wave: in pieces (above) when it has digests and its messages fit,
    // else the group form -- each group's RS right behind its upload, one
    // SHA-256 launch over every chunk, parity down group by group.
    int wave(std::vector<HostObj>& objs, size_t o0, size_t o1) {
        {
            uint64_t msgs = 0, up_bytes = 0, longest_msg = 0;
            for (size_t o = o0; o < o1; ++o) {
                for (int j = 0; j < objs[o].k; ++j) up_bytes += std::min<uint64_t>(objs[o].dlen[j], objs[o].S);
                if (!objs[o].dig) continue;
                msgs += uint64_t(objs[o].k + objs[o].m);
                longest_msg = std::max(longest_msg, objs[o].S);
            }
            const uint64_t P = piece_bytes(up_bytes, longest_msg);
            if (!watch_.shared_now()) piece_ramp_ = 0;  // a lone PUT keeps uniform pieces (the ramp cost it 5-9 %, piece_bytes)
            if (P && msgs && msgs <= lag_capacity()) return wave_pieces(objs, o0, o1, P);
        }
        uint8_t* base = static_cast<uint8_t*>(pool_.p);
        uint64_t msgs = 0;
        for (size_t o = o0; o < o1; ++o) msgs += uint64_t(objs[o].k + objs[o].m);
        MXEC_TRY(scratch_.grow(msgs * 32));
        uint8_t* digests = static_cast<uint8_t*>(scratch_.p);
        // Groups: consecutive objects up to kGroupBytes of input.
        std::vector<std::pair<size_t, size_t>> groups;
        for (size_t g0 = o0; g0 < o1;) {
            size_t g1 = g0;
            uint64_t in_bytes = 0;
            while (g1 < o1 && (g1 == g0 || in_bytes + uint64_t(objs[g1].k) * objs[g1].S <= kGroupBytes)) {
                in_bytes += uint64_t(objs[g1].k) * objs[g1].S;
                ++g1;
            }
            groups.emplace_back(g0, g1);
            g0 = g1;
        }
        // Phase 1: each group's upload and RS launch(es), in order.  The
        // host only waits on the input ring (an H2D copy), so uploads stream
        // at PCIe rate while RS runs behind them.
        std::vector<hipEvent_t> done(groups.size());
        bool any_dig = false;
        for (size_t o = o0; o < o1; ++o) any_dig = any_dig || objs[o].dig;
        hipStream_t rs_s = cs_[cs_idx_], sha_s = rs_s;
        // Each group's parity down: group by group after phase 1 (a lone
        // call queues all of phase 1 at once); while another call shares the
        // device, right behind the group's RS, since the paced phase 1 would
        // hold phase 3 back until the last uploads were queued.
        const bool down_early = watch_.shared_now();
        size_t downed = 0;
        auto down_group = [&](size_t g) -> int {
            MXEC_TRY(copy_.issue_down());
            MXEC_HIP(hipStreamWaitEvent(d2h_, done[g], 0));
            for (size_t o = groups[g].first; o < groups[g].second; ++o) {
                const HostObj& h = objs[o];
                uint8_t* ob = base + h.pool_off;
                for (int i = 0; i < h.m; ++i) {
                    MXEC_TRY(copy_.queue_down(h.parity[i], ob + uint64_t(h.k + i) * h.slot(), h.S));
                    if (h.S != h.slot()) MXEC_TRY(copy_.flush_down());
                }
            }
            MXEC_TRY(copy_.flush_down());  // before the next group's wait
            downed = g + 1;
            return MXEC_OK;
        };
        for (size_t g = 0; g < groups.size(); ++g) {
            watch_.open_up();
            const size_t g0 = groups[g].first, g1 = groups[g].second;
            for (size_t o = g0; o < g1; ++o) {
                const HostObj& h = objs[o];
                for (int j = 0; j < h.k; ++j) {
                    // a short chunk ends a run: the next chunk's slot does not follow its bytes
                    MXEC_TRY(copy_.queue_up(base + h.pool_off + uint64_t(j) * h.slot(), h.data[j], h.dlen[j]));
                    if (h.dlen[j] != h.slot()) MXEC_TRY(copy_.flush_up());
                }
            }
            MXEC_TRY(copy_.flush_up());
            hipEvent_t up;
            MXEC_TRY(copy_.new_event(&up));
            MXEC_TRY(copy_.new_event(&done[g]));
            MXEC_TRY(copy_.issue_up());
            MXEC_HIP(hipEventRecord(up, h2d_));
            MXEC_TRY(watch_.close_up());
            MXEC_HIP(hipStreamWaitEvent(rs_s, up, 0));
            MXEC_TRY(encode_piece(objs, g0, g1, 0, ~uint64_t(0), rs_s));
            MXEC_HIP(hipEventRecord(done[g], rs_s));
            if (down_early) MXEC_TRY(down_group(g));
            MXEC_TRY(copy_.pace(up));
        }
        copy_.end_pacing();
        // Phase 2: ONE SHA-256 launch over every chunk of the wave once all
        // parity exists.  A message's hash time does not depend on how many
        // messages share the launch (up to the split-form limit), so one
        // launch ends as early as any split of it would, and it needs no
        // more than one hardware queue.
        std::vector<const uint8_t*> sp;
        std::vector<uint64_t> sl;
        for (size_t o = o0; o < o1; ++o) {
            const HostObj& h = objs[o];
            if (!h.dig) continue;  // caller asked for no digests
            for (int j = 0; j < h.k + h.m; ++j) {
                sp.push_back(base + h.pool_off + uint64_t(j) * h.slot());
                sl.push_back(j < h.k ? std::min<uint64_t>(h.dlen[j], h.S) : h.S);
            }
        }
        hipEvent_t sha_done = nullptr;
        if (!sp.empty()) {
            MXEC_TRY(copy_.new_event(&sha_done));
            MXEC_HIP(hipStreamWaitEvent(sha_s, done.back(), 0));
            MXEC_TRY(run_sha(d_, slot_, sha_s, sp, sl, digests, nullptr, nullptr, nullptr, &arena_));
            MXEC_HIP(hipEventRecord(sha_done, sha_s));
        }
        // Phase 3: parity back group by group as RS finishes, digests last.
        for (size_t g = downed; g < groups.size(); ++g) MXEC_TRY(down_group(g));
        if (sha_done) {
            MXEC_TRY(digests_down(objs, o0, o1, digests, sha_done));
        }
        return copy_.flush();
    }
};

}  // namespace
}  // namespace mxec

using namespace mxec;

extern "C" int mxec_encode_batch_host(mxec_ctx* ctx, const mxec_object* objs, uint64_t n_obj,
                                      const uint8_t* const* data, const uint64_t* data_len,
                                      uint8_t* const* parity, uint8_t (*digests)[32],
                                      int32_t* status_out) {
    try {
        if (n_obj == 0) return MXEC_OK;
        if (!ctx || !objs || !data || !parity) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const size_t D = ctx->c.devs.size();
        if (!D) return set_error(MXEC_E_NO_DEVICE, "context has no device");
        uint64_t dsum = 0;
        for (uint64_t o = 0; o < n_obj; ++o) dsum += uint64_t(std::max(objs[o].k, 0));
        std::vector<uint64_t> dlen(size_t(dsum), 0);
        std::vector<std::vector<HostObj>> per(D);
        // Device of each object: o mod D for a uniform batch, balanced by
        // bytes for a mixed one (deal.hpp).
        std::vector<uint64_t> obj_bytes(size_t(n_obj), 0);
        for (uint64_t o = 0; o < n_obj; ++o)
            obj_bytes[o] = uint64_t(std::max(objs[o].k, 0) + std::max(objs[o].m, 0)) * rup(objs[o].shard_size, kAlign);
        std::vector<const void*> first(size_t(n_obj), nullptr);
        for (uint64_t o = 0, j = 0; o < n_obj; j += uint64_t(std::max(objs[o].k, 0)), ++o)
            if (objs[o].k > 0) first[o] = data[j];
        const std::vector<uint32_t> owner = deal_batch(ctx->c, obj_bytes, first);
        uint64_t doff = 0, poff = 0, goff = 0;
        int first_err = MXEC_OK;
        std::string first_msg;
        for (uint64_t o = 0; o < n_obj; ++o) {
            const int k = objs[o].k, m = objs[o].m;
            const uint64_t S = objs[o].shard_size;
            int st = check_km(k, m);
            if (st == MXEC_OK && S == 0) st = set_error(MXEC_E_EMPTY_SHARD, mxec_strerror(MXEC_E_EMPTY_SHARD));
            for (int j = 0; st == MXEC_OK && j < k; ++j) {
                const uint64_t l = data_len ? data_len[doff + uint64_t(j)] : S;
                if (l > S) st = set_error(MXEC_E_INCORRECT_SHARD_SIZE, "data chunk longer than shard_size");
                dlen[size_t(doff) + size_t(j)] = l;
            }
            if (status_out) status_out[o] = st;
            if (st != MXEC_OK) {
                if (first_err == MXEC_OK) {
                    first_err = st;
                    first_msg = last_error();
                }
            } else {
                HostObj h{k, m, S, data + doff, &dlen[size_t(doff)], parity + poff, digests ? digests + goff : nullptr};
                per[owner[o]].push_back(h);
            }
            doff += uint64_t(std::max(k, 0));
            poff += uint64_t(std::max(m, 0));
            goff += uint64_t(std::max(k, 0) + std::max(m, 0));
        }
        MXEC_TRY(for_each_device(ctx->c, per, [](Device& dev, PipeHub& hub, PipeLane& lane, std::vector<HostObj>& mine) {
            return PutCall(dev, hub, lane).run(mine);
        }));
        if (first_err != MXEC_OK) return set_error(first_err, first_msg);
        return MXEC_OK;
    } catch (const std::bad_alloc&) {
        return set_error(MXEC_E_OOM, "host allocation failed");
    } catch (const std::exception& e) {
        return set_error(MXEC_E_INVALID_ARG, e.what());
    }
}
