// Stand-alone harness for maxio_amd/csrc/frame_plan.hpp (the streaming
// encrypted PUT's arithmetic) and sha256_host.hpp (its frame AADs), built with
// -fsanitize=address,undefined by tests/test_writer_encrypted_abi.py.  One case
// per line on stdin, one answer line each:
//   len    plain              -> "frames stream_len" or "overflow"
//   frame  plain f            -> "stream_off stream_len plain_len"
//   due    plain from to      -> "first count" (the frames that become whole)
//   runs   plain from to      -> the launches due, "index:first_frame:frames:plain_len:stream_off:stream_len:last ..."
//   ring   chunk slots off len -> the ring stretches "slot:at:src:len ..." ("-" for none)
//   done   chunk total off len -> "first count" (the chunks the range completes)
//   aad    hex_prefix index   -> SHA-256(prefix || index as u64 LE) in hex ("-" = empty prefix)
// All numbers are unsigned 64-bit decimals.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../maxio_amd/csrc/frame_plan.hpp"
#include "../../maxio_amd/csrc/sha256_host.hpp"

using namespace mxec;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "len") {
            uint64_t plain = 0, total = 0;
            in >> plain;
            if (frame_stream_len(plain, &total)) std::printf("%" PRIu64 " %" PRIu64 "\n", frame_count(plain), total);
            else std::printf("overflow\n");
        } else if (op == "frame") {
            uint64_t plain = 0, f = 0;
            in >> plain >> f;
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", frame_stream_off(f), frame_stream_len_of(plain, f),
                        frame_plain_len(plain, f));
        } else if (op == "due") {
            uint64_t plain = 0, from = 0, to = 0;
            in >> plain >> from >> to;
            const FrameSpan s = frames_due(plain, from, to);
            std::printf("%" PRIu64 " %" PRIu64 "\n", s.first, s.count);
        } else if (op == "runs") {
            uint64_t plain = 0, from = 0, to = 0;
            in >> plain >> from >> to;
            int n = 0;
            const int rc = enc_runs_due(plain, from, to, [&](const EncRun& e) {
                std::printf("%s%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%d", n++ ? " " : "",
                            e.index, e.first_frame, e.frames, e.plain_len, e.stream_off, e.stream_len, int(e.last));
                return 0;
            });
            if (rc != 0) return 2;
            std::printf("%s\n", n ? "" : "-");
        } else if (op == "ring") {
            uint64_t c = 0, slots = 0, off = 0, len = 0, sum = 0;
            in >> c >> slots >> off >> len;
            int n = 0;
            const int rc = ring_segments(c, slots, off, len, [&](uint64_t slot, uint64_t at, uint64_t src, uint64_t m) {
                std::printf("%s%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64, n++ ? " " : "", slot, at, src, m);
                if (src != sum || m == 0 || at + m > c) return 1;
                sum += m;
                return 0;
            });
            if (rc != 0 || sum != len) return 2;
            std::printf("%s\n", n ? "" : "-");
        } else if (op == "done") {
            uint64_t c = 0, total = 0, off = 0, len = 0;
            in >> c >> total >> off >> len;
            const FrameSpan s = chunks_completed(c, total, off, len);
            std::printf("%" PRIu64 " %" PRIu64 "\n", s.first, s.count);
        } else if (op == "aad") {
            std::string hexs;
            uint64_t index = 0;
            in >> hexs >> index;
            std::vector<uint8_t> msg;
            if (hexs != "-")
                for (size_t i = 0; i + 1 < hexs.size(); i += 2) msg.push_back(uint8_t(std::stoi(hexs.substr(i, 2), nullptr, 16)));
            for (int b = 0; b < 8; ++b) msg.push_back(uint8_t(index >> (8 * b)));
            uint8_t d[32];
            sha256_host(msg.data(), msg.size(), d);
            for (int i = 0; i < 32; ++i) std::printf("%02x", d[i]);
            std::printf("\n");
        } else {
            return 3;
        }
    }
    return 0;
}
