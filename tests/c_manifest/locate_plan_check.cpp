// locate_plan_check — stand-alone driver of maxio_amd/csrc/locate_plan.hpp (the
// host side of mxec_locate: the per-(k, m) ratio -> shard table and
// mxec_locate_outcome's logic), built by tests/test_locate_abi.py with
// -fsanitize=address,undefined.
//
// Reads lines from stdin:
//   "raw K M b b b ..."      M x K parity rows, row-major
//   "out FIRST N MIN MAX"    a mxec_locate_result
// and prints per line "rc" followed, when rc == 0, by the table's 256
// ratio -> j entries and its M x K log-ratio entries; or "outcome shard".
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../maxio_amd/csrc/locate_plan.hpp"

int main() {
    static char buf[1 << 20];
    while (std::fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "out") {
            unsigned long long first = 0, n = 0;
            unsigned lo = 0, hi = 0;
            in >> first >> n >> lo >> hi;
            mxec_locate_result r{first, n, lo, hi};
            uint32_t shard = 0xDEAD;
            const int o = mxec::locate_outcome(&r, &shard);
            std::printf("%d %u\n", o, unsigned(shard));
            continue;
        }
        int k = 0, m = 0, b = 0;
        in >> k >> m;
        std::vector<uint8_t> rows;
        while (in >> b) rows.push_back(uint8_t(b));
        if (rows.size() != size_t(k > 0 ? k : 0) * size_t(m > 0 ? m : 0)) {
            std::printf("%d\n", MXEC_E_INVALID_ARG);
            continue;
        }
        // Exactly the bytes the builder may touch: the sanitizer sees a stray one.
        std::vector<uint8_t> tab(m >= 0 && m <= 8 ? mxec::locate_table_bytes(m) : 0);
        const int rc = mxec::locate_build_table(rows.data(), k, m, tab.data());
        std::printf("%d", rc);
        if (rc == 0) {
            for (int r = 0; r < 256; ++r) std::printf(" %u", unsigned(tab[size_t(r)]));
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < k; ++j) std::printf(" %u", unsigned(tab[size_t(256 * (1 + i) + j)]));
        }
        std::printf("\n");
    }
    return 0;
}
