// Stand-alone harness for the digest-run arithmetic of
// maxio_amd/csrc/writer_plan.hpp (SumRun, writer_sum_due, writer_sum_runs_of),
// built with -fsanitize=address,undefined by tests/test_sums_update_abi.py.
// One case per line on stdin, one answer line each:
//   due  chunk_size total_len chunk from to
//        -> the runs that become due when the chunk's uploaded bytes grow from
//           `from` to `to`: "at:len:first:last:closes ..." ("-" for none)
//   body chunk_size total_len step
//        -> the whole body in write() calls of `step` bytes, cut by writer_cut
//           and fed to writer_sum_due; checks that the runs tile every chunk
//           exactly once and in order, start on multiples of kSumRun, end on
//           one or on the chunk's end, and that the count is
//           writer_sum_runs_of's; prints "runs firsts lasts closes"
//   count chunk_size total_len chunk -> writer_sum_runs_of
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
        uint64_t c = 0, total = 0;
        in >> op >> c >> total;
        const WriterPlan p = WriterPlan::make(c, total, 0);
        if (op == "due") {
            uint64_t chunk = 0, from = 0, to = 0;
            in >> chunk >> from >> to;
            int n = 0;
            const int rc = writer_sum_due(p, chunk, from, to, [&](const SumRun& r) {
                if (r.chunk != chunk) return 4;
                std::printf("%s%" PRIu64 ":%" PRIu64 ":%d:%d:%d", n++ ? " " : "", r.at, r.len, int(r.first), int(r.last),
                            int(r.closes));
                return 0;
            });
            if (rc) return rc;
            std::printf("%s\n", n ? "" : "-");
        } else if (op == "body") {
            uint64_t step = 0;
            in >> step;
            uint64_t runs = 0, firsts = 0, lasts = 0, closes = 0;
            uint64_t chunk = 0, covered = 0, in_chunk = 0;  // the next run must start at `covered` of `chunk`
            auto take = [&](const SumRun& r) {
                if (r.chunk != chunk || r.at != covered) return 5;            // in order, no gap, no overlap
                if (r.at % kSumRun) return 6;                                  // starts on a mark
                const uint64_t len = p.chunk_len(r.chunk);
                if (r.len > kSumRun || r.len > len - r.at) return 7;          // stays inside the chunk
                const uint64_t end = r.at + r.len;
                if (end != len && end % kSumRun) return 8;                    // ends on a mark or the chunk's end
                if (r.closes != (end == len)) return 9;
                if (r.first != (runs == 0)) return 10;
                if (r.last != (r.closes && r.chunk + 1 == p.k)) return 11;
                ++runs, ++in_chunk;
                firsts += r.first, lasts += r.last, closes += r.closes;
                covered = end;
                if (r.closes) {
                    if (in_chunk != writer_sum_runs_of(p, r.chunk)) return 12;
                    ++chunk, covered = 0, in_chunk = 0;
                }
                return 0;
            };
            int rc = 0;
            if (total == 0) rc = writer_sum_due(p, 0, 0, 0, take);  // finish()'s one empty run
            for (uint64_t written = 0; !rc && written < total;) {
                const uint64_t len = total - written < step ? total - written : step;
                rc = writer_cut(p, written, len, [&](const WriterRun& r) {
                    return writer_sum_due(p, r.chunk, r.at, r.at + r.len, take);
                });
                written += len;
            }
            if (rc) return rc;
            if (chunk != p.k) return 13;  // every chunk closed
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", runs, firsts, lasts, closes);
        } else if (op == "count") {
            uint64_t chunk = 0;
            in >> chunk;
            std::printf("%" PRIu64 "\n", writer_sum_runs_of(p, chunk));
        } else {
            return 3;
        }
    }
    return 0;
}
