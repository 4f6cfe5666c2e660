// rs_args.hpp — what one launch of the Reed-Solomon kernels (rs_kernel.hip) is
// handed: the argument block and the records its tables hold.  Plain data, no
// HIP: kernels.hpp includes it for the launchers, rs_plan.hpp for the host
// planner that fills it (and, through that, the stand-alone CPU check
// tests/c_manifest/rs_plan_check.cpp).
#pragma once

#include <cstdint>

namespace mxec {

// One launch applies an r x k GF(2^8) matrix to a batch of objects that share
// (k, r, shard_size):  out[o][i][b] = XOR_j coef(o)[i][j] * in[o][j][b].
// Bytes of input j at or beyond in_len[o][j] read as zero (the crate's
// zero padding, filesystem.rs:1111 / chunk_reader.rs:192); output i is written
// for b < out_len[o][i] only.
struct alignas(16) RsTileRec {  // one tile of a grouped launch (below)
    uint32_t obj;    // its object
    uint32_t k;      // the object's input count
    uint32_t in0;    // the object's first entry in in_ptrs / in_len
    uint32_t local;  // the tile's index within the object
};
// One object's result of a locate launch (mxec_locate_result's layout).
struct LocateRec {
    uint64_t first_bad;  // lowest bad byte column (atomic min)
    uint64_t n_bad;      // bad byte columns (atomic add)
    uint32_t shard_min;  // min / max of the columns' candidate shards
    uint32_t shard_max;
};
constexpr uint32_t kLocateNoShard = 0xFFFFFFFEu;
struct RsArgs {
    const uint8_t* const* in_ptrs;  // [n_obj][k]
    uint8_t* const* out_ptrs;       // [n_obj][r_total]; this launch writes rows
                                    //   [row0, row0 + r)
    const uint64_t* in_len;         // [n_obj][k]
    const uint64_t* out_len;        // [n_obj][r_total]
    const uint32_t* coef;           // tables, [j][i][8] per matrix (gf256.hpp)
    const uint32_t* coef_off;       // [n_obj] dword offset of object's table
    const uint64_t* edge_list;      // [n_edge] object << 32 | tile: every tile
                                    //   of an unaligned launch (edge kernel)
    uint64_t n_edge;
    uint64_t edge_tile_bytes;       // tile size the list was built for
    uint64_t shard_size;
    uint32_t n_obj, k, r, r_total, row0;
    uint32_t aligned;               // all pointers 16-byte aligned (else every
                                    //   tile is in the edge list)
    // Grouped launch (objects of different k and shard size sharing r, every
    // pointer aligned, r_total == r <= 8): when `tiles` is set, launch tile t
    // is tiles[t] — its object, that object's k and first input entry, and
    // the tile's index within the object.  k and shard_size above are then
    // unused.
    const RsTileRec* tiles = nullptr;
    uint64_t n_tiles = 0;
    // Multi-r grouped launch (tiles set): objects of every r <= kMultiR in
    // one grid; tiles[t].k holds k | r << 16, object o's outputs are
    // out_ptrs / out_len [o * kMultiR, o * kMultiR + r), its coefficient
    // table rows r apart.  r, r_total and row0 above are unused.
    uint32_t multi = 0;
    // Uniform launches: workgroups per CU chosen by the caller (the grid
    // tuner, ops.cpp); 0 = rs_default_variant's.
    uint32_t blocks_per_cu = 0;
    // Every launch form: at most this many workgroups (0: no cap).  Tests
    // (mxec_open_test rs_grid_cap) shrink the grid so each workgroup walks many tiles.
    uint32_t max_blocks = 0;
    // Verify launch (ReedSolomon::verify) when set: nothing is written to
    // out_ptrs -- they are the stored parity rows, read and compared with the
    // recomputed ones -- and first_bad[o] points at object o's r_total
    // entries: entry i receives (atomic min) the lowest byte offset at which
    // stored row i differs, and is left alone when the row agrees.  The
    // caller fills the entries with 0xFF on the stream ahead of the launch.
    // Not with `multi`.
    uint64_t* const* first_bad = nullptr;
    // Locate launch (mxec_locate) when set, instead of first_bad: the verify's
    // walk (r == r_total <= 8, one row block), but a wave that finds a
    // mismatch classifies each bad byte column and folds the result into
    // locate[o], object o's record (initialised by launch_locate_init on the
    // stream ahead of the launch).  loc_field: the field's log / exp tables,
    // loc_tab + loc_off[o]: object o's (k, m) table (locate_plan.hpp); all
    // three in device memory, uploaded with the descriptor tables.
    LocateRec* const* locate = nullptr;
    const uint8_t* loc_field = nullptr;
    const uint8_t* loc_tab = nullptr;
    const uint32_t* loc_off = nullptr;
    // Seeded launch (mxec_encode_update_strided_device) when set: a uniform
    // store launch whose accumulators start from seed rows instead of zero,
    // out = seed ^ coef * in.  [n_obj][r_total] like out_ptrs, read at
    // [row0, row0 + r) and cut at out_len like the rows written.  nullptr is
    // the plain launch, bit for bit.  The seed rows and the output rows are
    // different buffers, by contract: with_stable_coef (ops.hpp) may queue a
    // batch again over the same outputs and relies on the kernels reading only
    // inputs and writing only outputs -- a read-modify-write of one buffer
    // would fold the window in twice.  Reading seed_ptrs and writing out_ptrs,
    // a re-run is exact.  Not with tiles, first_bad or locate.
    const uint8_t* const* seed_ptrs = nullptr;
};
constexpr uint32_t kMultiR = 4;

}  // namespace mxec
