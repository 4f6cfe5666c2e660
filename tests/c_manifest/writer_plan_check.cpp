// Stand-alone harness for maxio_amd/csrc/writer_plan.hpp (the streaming PUT's
// arithmetic), built with -fsanitize=address,undefined by
// tests/test_writer_abi.py.  One case per line on stdin, one answer line each:
//   plan  chunk_size total_len window_bytes          -> "k last_len slots"
//   cut   chunk_size total_len window_bytes written len
//         -> "overrun: <message>" or the runs "chunk:at:src:len:opens:completes ..." ("-" for none)
//   slots chunk_size total_len window_bytes n        -> for chunks 0..n-1 "slot/evicts" ("-" = no wait)
//   end   chunk_size total_len written               -> "ok" or the short-finish message
// All numbers are unsigned 64-bit decimals.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../maxio_amd/csrc/writer_plan.hpp"

using namespace mxec;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        uint64_t c = 0, total = 0, win = 0;
        in >> op >> c >> total;
        if (op == "end") {
            uint64_t written = 0;
            in >> written;
            const WriterPlan p = WriterPlan::make(c, total, 0);
            std::printf("%s\n", written == p.total_len ? "ok" : writer_short_msg(p, written).c_str());
            continue;
        }
        in >> win;
        const WriterPlan p = WriterPlan::make(c, total, win);
        if (op == "plan") {
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p.k, p.chunk_len(p.k - 1), p.slots);
        } else if (op == "cut") {
            uint64_t written = 0, len = 0;
            in >> written >> len;
            if (writer_overruns(p, written, len)) {
                std::printf("overrun: %s\n", writer_overrun_msg(p, written, len).c_str());
                continue;
            }
            int n = 0;
            uint64_t sum = 0;
            const int rc = writer_cut(p, written, len, [&](const WriterRun& r) {
                std::printf("%s%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%d:%d", n++ ? " " : "", r.chunk, r.at, r.src,
                            r.len, int(r.opens), int(r.completes));
                sum += r.len;
                return 0;
            });
            if (rc != 0 || sum != len) return 2;
            std::printf("%s\n", n ? "" : "-");
        } else if (op == "slots") {
            uint64_t n = 0;
            in >> n;
            for (uint64_t j = 0; j < n; ++j) {
                std::printf("%s%" PRIu64 "/", j ? " " : "", p.slot_of(j));
                if (p.reuses(j)) std::printf("%" PRIu64, p.evicts(j));
                else std::printf("-");
            }
            std::printf("\n");
        } else {
            return 3;
        }
    }
    return 0;
}
