// scrub_plan_check — stand-alone driver of maxio_amd/csrc/scrub_plan.hpp (the
// states -> damaged count -> verdict logic of mxec_scrub_object), built by
// tests/test_verify_abi.py with -fsanitize=address,undefined.
//
// Reads lines "m heal parity_consistent rebuilt_ok state state ..." from
// stdin and prints "n_damaged can_heal verdict" for each.
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../../maxio_amd/csrc/scrub_plan.hpp"

int main() {
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        std::istringstream in(line);
        unsigned m = 0;
        int heal = 0, pc = 0, rebuilt = 0, s = 0;
        if (!(in >> m >> heal >> pc >> rebuilt)) continue;
        std::vector<uint8_t> st;
        while (in >> s) st.push_back(uint8_t(s));
        const uint32_t nd = mxec::scrub_damaged(st.data(), uint32_t(st.size()));
        std::printf("%u %d %u\n", nd, mxec::scrub_can_heal(nd, m) ? 1 : 0,
                    mxec::scrub_verdict(nd, m, pc, heal != 0, rebuilt != 0));
    }
    return 0;
}
