// storage_put.cpp — the write side of MaxIO's FilesystemStorage at the file
// level, over the GPU encode / hash entry points:
//   write_chunk                  filesystem.rs:1062-1080
//   compute_and_write_parity     filesystem.rs:1084-1145
//   put_object_chunked (body)    filesystem.rs:686-773 (chunking + manifest)
// and the encrypt-then-EC and multipart drivers built on them.
// Differences in *how*, not *what*: data digests of a whole body are computed
// in one GPU batch instead of chunk by chunk, and parity is encoded from the
// body already in memory instead of re-reading the data chunk files
// (:1108-1113).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <future>

#include "ops.hpp"
#include "shard_files.hpp"

using namespace mxec;

namespace {

void fill_info(mxec_chunk_info* ci, uint32_t index, uint64_t size, const uint8_t* digest, uint8_t kind) {
    ci->index = index;
    ci->size = size;
    std::memcpy(ci->sha256, hex(digest, 32).c_str(), 65);
    ci->kind = kind;
}

// m parity shards of chunk_size bytes for the k data chunks (the encode
// writes every byte: no zero-fill) and the k+m digests.
int encode_parity(mxec_ctx* ctx, uint64_t chunk_size, const std::vector<const uint8_t*>& dp,
                  const std::vector<size_t>& dl, int m, std::vector<Bytes>& parity, std::vector<uint8_t>& dig) {
    parity.resize(size_t(m > 0 ? m : 0));
    std::vector<uint8_t*> pp;
    for (auto& b : parity) {
        b.resize(chunk_size);
        pp.push_back(b.data());
    }
    dig.resize((dp.size() + parity.size()) * 32);
    return mxec_encode(ctx, int(dp.size()), m, chunk_size, dp.data(), dl.data(), pp.data(),
                       reinterpret_cast<uint8_t(*)[32]>(dig.data()));
}

// Md5 / ChecksumHasher over the plaintext (:722-725, :878-884): the reference
// feeds them as the body arrives; here one batched pass after the PUT.
int body_sums(mxec_ctx* ctx, const uint8_t* body, size_t len, uint32_t which, mxec_body_sums* out) {
    if (!which) return MXEC_OK;
    const uint8_t* b = body ? body : reinterpret_cast<const uint8_t*>("");
    const uint64_t l = len;
    return mxec_body_sums_batch(ctx, &b, &l, 1, which, out);
}

}  // namespace

extern "C" {

int mxec_write_chunk(mxec_ctx* ctx, const char* ec_dir, uint32_t index, const uint8_t* data, size_t len,
                     mxec_chunk_info* out) {
    return guarded([&]() -> int {
        if (!ec_dir || !out || (len && !data)) return set_error(MXEC_E_INVALID_ARG, "null argument");
        uint8_t dig[1][32];
        const uint8_t* b = data ? data : reinterpret_cast<const uint8_t*>("");
        MXEC_TRY(mxec_sha256_batch(ctx, &b, &len, 1, dig));
        MXEC_TRY(write_file(fs::path(ec_dir) / chunk_name(index), data, len));
        fill_info(out, index, len, dig[0], 0);
        return MXEC_OK;
    });
}

int mxec_compute_and_write_parity(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                  uint32_t parity_shards, const mxec_chunk_info* data_chunks, int k,
                                  mxec_chunk_info* parity_out) {
    return guarded([&]() -> int {
        if (!ec_dir || (k > 0 && !data_chunks) || !parity_out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        const int m = int(parity_shards);
        if (k + m > 255) return too_many_shards(k, m);
        const fs::path dir(ec_dir);
        std::vector<Bytes> data(static_cast<size_t>(k));
        std::vector<const uint8_t*> dp(static_cast<size_t>(k));
        std::vector<size_t> dl(static_cast<size_t>(k));
        for (int j = 0; j < k; ++j) {
            MXEC_TRY(read_file(dir / chunk_name(data_chunks[j].index), data[size_t(j)]));
            if (data[size_t(j)].size() > chunk_size) data[size_t(j)].resize(chunk_size);  // Vec::resize
            dp[size_t(j)] = data[size_t(j)].data();
            dl[size_t(j)] = data[size_t(j)].size();
        }
        std::vector<Bytes> parity;
        std::vector<uint8_t> dig;
        MXEC_TRY(encode_parity(ctx, chunk_size, dp, dl, m, parity, dig));
        for (int i = 0; i < m; ++i) {
            MXEC_TRY(write_file(dir / chunk_name(uint32_t(k + i)), parity[size_t(i)].data(), chunk_size));
            fill_info(&parity_out[i], uint32_t(k + i), chunk_size, &dig[size_t(k + i) * 32], 1);
        }
        return MXEC_OK;
    });
}

}  // extern "C"

namespace {

// put_object_chunked's chunking, chunk files, parity and manifest for a
// buffered body (filesystem.rs:686-828).  plain_size >= 0 records
// manifest.plaintext_size: the encrypt-then-EC drivers chunk the frame
// stream and keep the plaintext length (:973-990, :1472-1486).
int put_chunked_buffer(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                       const uint8_t* body, size_t len, int64_t plain_size) {
    if (!ec_dir || (len && !body)) return set_error(MXEC_E_INVALID_ARG, "null argument");
    if (chunk_size == 0) return set_error(MXEC_E_INVALID_ARG, "chunk_size must be > 0");
    const fs::path dir(ec_dir);
    std::error_code ec;
    fs::create_directories(dir, ec);
    if (ec) return set_error(MXEC_E_IO, "IO error: " + ec.message());
    // Chunking (:709-737): full chunk_size slices, final partial unpadded;
    // empty body -> one empty chunk (:740-743).
    std::vector<const uint8_t*> dp;
    std::vector<size_t> dl;
    for (size_t off = 0; off < len; off += chunk_size) {
        dp.push_back(body + off);
        dl.push_back(size_t(std::min<uint64_t>(chunk_size, len - off)));
    }
    static const uint8_t empty = 0;
    if (dp.empty()) {
        dp.push_back(&empty);
        dl.push_back(0);
    }
    const int k = int(dp.size());
    const bool has_parity = parity_shards > 0 && len > 0;  // :748
    const int m = has_parity ? int(parity_shards) : 0;
    auto write_data = [&]() -> int {
        for (int j = 0; j < k; ++j) MXEC_TRY(write_file(dir / chunk_name(uint32_t(j)), dp[size_t(j)], dl[size_t(j)]));
        return MXEC_OK;
    };
    std::vector<uint8_t> dig(size_t(k) * 32);
    if (has_parity && k + m > 255) {
        // The reference writes the data chunks first (write_chunk), then
        // hits the k+m guard inside compute_and_write_parity.
        MXEC_TRY(write_data());
        return too_many_shards(k, m);
    } else if (has_parity) {
        // The data chunk files are written on a helper thread while the
        // device encodes and hashes (the ~30 ms SHA-256 chain of a 1 MiB
        // chunk hides the writes); a write error still wins over anything
        // the encode reports, as the reference writes them first.
        // The future's destructor joins the thread on every path.
        auto writer = std::async(std::launch::async, [&]() -> std::pair<int, std::string> {
            try {
                const int rc = write_data();
                return {rc, rc ? last_error() : ""};
            } catch (...) {
                return {MXEC_E_IO, "IO error: data chunk write failed"};
            }
        });
        std::vector<Bytes> parity;
        const int erc = encode_parity(ctx, chunk_size, dp, dl, m, parity, dig);
        const std::string emsg = erc ? std::string(last_error()) : std::string();
        const auto [wrc, wmsg] = writer.get();
        if (wrc) return set_error(wrc, wmsg);
        if (erc) return set_error(erc, emsg);
        for (int i = 0; i < m; ++i)
            MXEC_TRY(write_file(dir / chunk_name(uint32_t(k + i)), parity[size_t(i)].data(), chunk_size));
    } else {
        MXEC_TRY(mxec_sha256_batch(ctx, dp.data(), dl.data(), size_t(k), reinterpret_cast<uint8_t(*)[32]>(dig.data())));
        MXEC_TRY(write_data());
    }
    Manifest man;
    man.version = has_parity ? 2 : 1;
    man.total_size = len;
    man.chunk_size = chunk_size;
    man.chunk_count = uint32_t(k);
    for (int j = 0; j < k + m; ++j) {
        man.chunks.push_back({uint32_t(j), j < k ? dl[size_t(j)] : chunk_size, hex(&dig[size_t(j) * 32], 32),
                              uint8_t(j < k ? 0 : 1)});  // index, size, sha256, kind
    }
    man.has_parity = man.has_shard = has_parity;  // the Option fields: written only when Some
    man.parity_shards = parity_shards;
    man.shard_size = chunk_size;
    man.has_plain = plain_size >= 0;
    man.plaintext_size = uint64_t(plain_size);
    const std::string js = manifest_json(man);
    return write_file(dir / "manifest.json", reinterpret_cast<const uint8_t*>(js.data()), js.size());
}

// AES-256-GCM frame stream of `pt` under `key` (crypto.rs FrameEncryptor,
// 64 KiB frames, first index 0), frame i's AAD = SHA-256(aad_prefix || i LE)
// (build_frame_aad, filesystem.rs:118-128).
int encrypt_frames(mxec_ctx* ctx, const uint8_t* key, const uint8_t* nonce_prefix, const uint8_t* aad_prefix,
                   uint32_t aad_prefix_len, const uint8_t* pt, uint64_t len, std::vector<uint8_t>& ct) {
    const uint64_t nf = (len + MXEC_FRAME_CHUNK_SIZE - 1) / MXEC_FRAME_CHUNK_SIZE;
    ct.assign(size_t(mxec_frames_len(len, MXEC_FRAME_CHUNK_SIZE)), 0);
    if (nf == 0) return MXEC_OK;
    std::vector<uint8_t> aads(size_t(nf) * 32);
    MXEC_TRY(mxec_frame_aads(ctx, aad_prefix, aad_prefix_len, 0, nf, reinterpret_cast<uint8_t(*)[32]>(aads.data())));
    uint64_t n = 0;
    MXEC_TRY(mxec_frames_encrypt(ctx, key, nonce_prefix, 0, aads.data(), 32, MXEC_FRAME_CHUNK_SIZE, pt, len,
                                 ct.data(), ct.size(), &n));
    ct.resize(size_t(n));
    return MXEC_OK;
}

// The parts of a multipart upload concatenated in order (plaintext).  An
// encrypted part is a frame stream under the upload key with AADs
// SHA-256("PART" 0 upload_id 0 part_number_le4 0 || i LE) (part_aad_builder,
// filesystem.rs:147-163), decrypted by FrameDecryptor (:1378-1388).
int read_parts(mxec_ctx* ctx, const mxec_multipart_part* parts, uint32_t n_parts, const uint8_t* upload_key,
               const char* upload_id, std::vector<uint8_t>& out) {
    out.clear();
    for (uint32_t p = 0; p < n_parts; ++p) {
        const mxec_multipart_part& part = parts[p];
        if (!part.path) return set_error(MXEC_E_INVALID_ARG, "null part path");
        Bytes raw;
        MXEC_TRY(read_file(part.path, raw));
        if (!part.encrypted) {
            out.insert(out.end(), raw.begin(), raw.end());
            continue;
        }
        if (!upload_key || !upload_id) return set_error(MXEC_E_INVALID_ARG, "encrypted part without upload key");
        std::string prefix = std::string("PART") + '\0' + upload_id + '\0';
        for (int b = 0; b < 4; ++b) prefix.push_back(char((part.part_number >> (8 * b)) & 0xFF));
        prefix.push_back('\0');
        const uint64_t nf = (part.size + MXEC_FRAME_CHUNK_SIZE - 1) / MXEC_FRAME_CHUNK_SIZE;
        std::vector<uint8_t> aads(size_t(nf) * 32 + 32);
        if (nf)
            MXEC_TRY(mxec_frame_aads(ctx, reinterpret_cast<const uint8_t*>(prefix.data()), uint32_t(prefix.size()), 0,
                                     nf, reinterpret_cast<uint8_t(*)[32]>(aads.data())));
        const size_t at = out.size();
        out.resize(at + size_t(part.size));
        uint64_t n = 0;
        MXEC_TRY(mxec_frames_decrypt(ctx, upload_key, 0, aads.data(), 32, MXEC_FRAME_CHUNK_SIZE, raw.data(),
                                     raw.size(), part.size, out.data() + at, part.size, &n));
        if (n != part.size) return set_error(MXEC_E_INTEGRITY, "part plaintext size mismatch");
    }
    return MXEC_OK;
}

}  // namespace

extern "C" {

int mxec_put_object_chunked(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                            const uint8_t* body, size_t len) {
    return guarded([&]() -> int {
        return put_chunked_buffer(ctx, ec_dir, chunk_size, parity_shards, body, len, -1);
    });
}

int mxec_put_object_chunked_sums(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size, uint32_t parity_shards,
                                 const uint8_t* body, size_t len, uint32_t which, mxec_body_sums* sums_out) {
    return guarded([&]() -> int {
        if (which && !sums_out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        MXEC_TRY(mxec_put_object_chunked(ctx, ec_dir, chunk_size, parity_shards, body, len));
        return body_sums(ctx, body, len, which, sums_out);
    });
}

int mxec_put_object_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                      uint32_t parity_shards, const uint8_t key[32], const uint8_t nonce_prefix[4],
                                      const uint8_t* aad_prefix, uint32_t aad_prefix_len, const uint8_t* body,
                                      size_t len, uint32_t which, mxec_body_sums* sums_out) {
    return guarded([&]() -> int {
        if (!key || !nonce_prefix || (len && !body) || (aad_prefix_len && !aad_prefix) || (which && !sums_out))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        std::vector<uint8_t> ct;
        MXEC_TRY(encrypt_frames(ctx, key, nonce_prefix, aad_prefix, aad_prefix_len, body, len, ct));
        MXEC_TRY(put_chunked_buffer(ctx, ec_dir, chunk_size, parity_shards, ct.data(), ct.size(), int64_t(len)));
        return body_sums(ctx, body, len, which, sums_out);
    });
}

int mxec_complete_multipart_chunked(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                    uint32_t parity_shards, const mxec_multipart_part* parts, uint32_t n_parts,
                                    char etag_out[48]) {
    return guarded([&]() -> int {
        if ((n_parts && !parts) || !etag_out) return set_error(MXEC_E_INVALID_ARG, "null argument");
        std::vector<uint8_t> body;
        for (uint32_t p = 0; p < n_parts; ++p)
            if (parts[p].encrypted) return set_error(MXEC_E_INVALID_ARG, "encrypted part: use the _encrypted driver");
        MXEC_TRY(read_parts(ctx, parts, n_parts, nullptr, nullptr, body));
        MXEC_TRY(put_chunked_buffer(ctx, ec_dir, chunk_size, parity_shards, body.data(), body.size(), -1));
        return multipart_etag(ctx, parts, n_parts, etag_out);
    });
}

int mxec_complete_multipart_chunked_encrypted(mxec_ctx* ctx, const char* ec_dir, uint64_t chunk_size,
                                              uint32_t parity_shards, const mxec_multipart_part* parts,
                                              uint32_t n_parts, const uint8_t upload_key[32], const char* upload_id,
                                              const uint8_t key[32], const uint8_t nonce_prefix[4],
                                              const uint8_t* aad_prefix, uint32_t aad_prefix_len,
                                              char etag_out[48]) {
    return guarded([&]() -> int {
        if ((n_parts && !parts) || !etag_out || !key || !nonce_prefix || (aad_prefix_len && !aad_prefix))
            return set_error(MXEC_E_INVALID_ARG, "null argument");
        std::vector<uint8_t> plain, ct;
        MXEC_TRY(read_parts(ctx, parts, n_parts, upload_key, upload_id, plain));
        MXEC_TRY(encrypt_frames(ctx, key, nonce_prefix, aad_prefix, aad_prefix_len, plain.data(), plain.size(), ct));
        MXEC_TRY(put_chunked_buffer(ctx, ec_dir, chunk_size, parity_shards, ct.data(), ct.size(), int64_t(plain.size())));
        return multipart_etag(ctx, parts, n_parts, etag_out);
    });
}

}  // extern "C"
