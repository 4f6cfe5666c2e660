// shard_files_check — stand-alone driver of maxio_amd/csrc/shard_files.cpp
// (the storage entry points' file I/O), built by tests/test_shard_files.py
// with -fsanitize=address,undefined together with manifest.cpp.
//
//   shard_files_check DIR      DIR: an empty scratch directory
// Prints one line per failed check and "shard_files_check ok" when none failed.
#include <cctype>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../maxio_amd/csrc/shard_files.hpp"

namespace mxec {
static thread_local std::string g_error;
int set_error(int code, const std::string& msg) {
    g_error = msg;
    return code;
}
const char* last_error() { return g_error.c_str(); }
}  // namespace mxec

using namespace mxec;

static int failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, last_error()); \
            ++failed;                                                      \
        }                                                                  \
    } while (0)

static Bytes pattern(size_t n, unsigned seed) {
    Bytes b(n);
    for (size_t i = 0; i < n; ++i) b[i] = uint8_t((i * 131 + seed) >> 3);
    return b;
}

static std::vector<std::string> names(const fs::path& dir) {
    std::vector<std::string> out;
    for (const auto& e : fs::directory_iterator(dir)) out.push_back(e.path().filename().string());
    return out;
}

static void put_text(const fs::path& p, const std::string& s) { std::ofstream(p, std::ios::binary) << s; }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const fs::path dir(argv[1]);

    // write_file / read_file; 300 000 bytes come from BigPool, the second
    // time from its free list.
    for (size_t n : {size_t(0), size_t(1), size_t(300000), size_t(300000)}) {
        const Bytes want = pattern(n, unsigned(n));
        CHECK(write_file(dir / "rt", want.data(), n) == MXEC_OK);
        Bytes got = pattern(7, 1);  // replaced whole, whatever it held
        CHECK(read_file(dir / "rt", got) == MXEC_OK);
        CHECK(got == want);
    }
    Bytes none;
    CHECK(read_file(dir / "absent", none) == MXEC_E_IO && std::strstr(last_error(), "IO error: "));

    // read_file_to: the right size, a wrong one (destination untouched), no file.
    const Bytes body = pattern(1000, 3);
    CHECK(write_file(dir / "to", body.data(), body.size()) == MXEC_OK);
    Bytes dst(1000, 0xEE);
    uint64_t size = 0;
    CHECK(read_file_to(dir / "to", dst.data(), 1000, &size) == MXEC_OK && size == 1000 && dst == body);
    dst.assign(1000, 0xEE);
    size = 0;
    CHECK(read_file_to(dir / "to", dst.data(), 999, &size) == MXEC_OK && size == 1000);
    CHECK(dst == Bytes(1000, 0xEE));
    CHECK(read_file_to(dir / "absent", dst.data(), 1000, &size) == MXEC_E_IO);

    // replace_file: the new bytes under the final name, no temporary left.
    const fs::path heal = dir / "heal";
    fs::create_directory(heal);
    CHECK(write_file(heal / "000001", body.data(), 10) == MXEC_OK);
    CHECK(replace_file(heal, "000001", body.data(), body.size()) == MXEC_OK);
    Bytes healed;
    CHECK(read_file(heal / "000001", healed) == MXEC_OK && healed == body);
    CHECK(names(heal) == std::vector<std::string>{"000001"});
    CHECK(replace_file(dir / "nowhere", "000001", body.data(), body.size()) == MXEC_E_IO);
    CHECK(!fs::exists(dir / "nowhere"));

    // hex / unhex32.
    uint8_t raw[32], back[32];
    for (int i = 0; i < 32; ++i) raw[i] = uint8_t(i * 9 + 0xA0);
    const std::string h = hex(raw, 32);
    CHECK(h.size() == 64 && h.substr(0, 6) == "a0a9b2" && hex(raw, 16) == h.substr(0, 32) && hex(raw, 0).empty());
    CHECK(unhex32(h, back) && std::memcmp(raw, back, 32) == 0);
    std::string upper = h;
    for (char& c : upper) c = char(std::toupper(c));
    CHECK(unhex32(upper, back) && std::memcmp(raw, back, 32) == 0);
    CHECK(!unhex32(h.substr(0, 63), back));
    CHECK(!unhex32(h.substr(0, 63) + "g", back));
    // manifest_digest32: only what hex() writes (the reference compares strings).
    std::memset(back, 0, 32);
    CHECK(manifest_digest32(h, back) && std::memcmp(raw, back, 32) == 0);
    std::string one_upper = h;
    one_upper[0] = 'A';
    CHECK(!manifest_digest32(upper, back) && !manifest_digest32(one_upper, back));
    CHECK(!manifest_digest32(h.substr(0, 63), back) && !manifest_digest32(h + "0", back));
    CHECK(chunk_name(7) == "000007" && chunk_name(1234567) == "1234567");

    // read_manifest: what it accepts, bytes that are not UTF-8, chunks
    // shorter than chunk_count.
    const std::string chunk = "{\"index\": 0, \"size\": 10, \"sha256\": \"" + h + "\"}";
    const std::string head = "{\"version\": 1, \"total_size\": 20, \"chunk_size\": 10, \"chunk_count\": 2, \"chunks\": [";
    Manifest man;
    put_text(dir / "manifest.json", head + chunk + ", " + chunk + "]}");
    CHECK(read_manifest(dir, man) == MXEC_OK && man.chunk_count == 2 && man.chunks.size() == 2);
    put_text(dir / "manifest.json", head + chunk + "]}");
    CHECK(read_manifest(dir, man) == MXEC_E_JSON && std::strstr(last_error(), "fewer chunks than chunk_count"));
    put_text(dir / "manifest.json", head + chunk + ", " + chunk + "]} \xC0\xAF");
    CHECK(read_manifest(dir, man) == MXEC_E_IO && std::strstr(last_error(), "valid UTF-8"));
    CHECK(read_manifest(dir / "nowhere", man) == MXEC_E_IO);

    if (!failed) std::printf("shard_files_check ok\n");
    return failed ? 1 : 0;
}
