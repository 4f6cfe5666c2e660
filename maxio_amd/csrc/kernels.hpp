// kernels.hpp — launch interface of the gfx950 kernels (rs_kernel.hip,
// sha256_kernel.hip).  Host code builds the descriptor tables in device
// memory and calls these launchers on a HIP stream.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/maxio_ec.h"
#include "rs_args.hpp"

namespace mxec {

// The RS launch argument block (RsArgs) and the records its tables hold
// (RsTileRec, LocateRec, kLocateNoShard, kMultiR): rs_args.hpp, plain data
// that the host-only planner rs_plan.hpp shares.

// n records to the clean pattern {~0, 0, ~0, 0}.
hipError_t launch_locate_init(LocateRec* recs, uint64_t n, hipStream_t s);

// Geometry of a launch of the interior kernel (tools/kernel_lab.cpp sweeps
// the grid).
struct RsVariant {
    int vecs = 2;           // 16-byte column vectors per lane per tile: 4 for r_total <= 4, else 2
    int blocks_per_cu = 8;  // grid = n_cus * blocks_per_cu (grid-stride)
};

// Uniform launches, or grouped ones (a.tiles set: rs_group_variant, aligned).
hipError_t launch_rs_apply(const RsArgs& a, int n_cus, hipStream_t s);
hipError_t launch_rs_apply_variant(const RsArgs& a, int n_cus, hipStream_t s, const RsVariant& v);
// Geometry the default launch uses for a given total row count, and its tile.
RsVariant rs_default_variant(uint32_t r_total);
// Geometry of grouped launches (a.tiles set) for r rows.
RsVariant rs_group_variant(uint32_t r);
uint64_t rs_tile_bytes(const RsVariant& v);

// SHA-256 over n messages, one lane per message.  If `expected` is set the
// kernel also writes ok[i] = (digest == expected[i]).
// Piece mode of the lag pair form (the host pipeline hashes every chunk piece by
// piece while later pieces still upload): launch message i is the next piece
// of the chain kept in state slot slot[i].  With resume the chain continues
// from state[slot] (else from the IV).  total[i] == kShaNotFinal: the piece
// ends mid-message (a multiple of 64 bytes) and the running state goes back
// to state[slot]; otherwise it is the last piece of a total[i]-byte message,
// padded and finished into digests[slot] (ok[slot] against
// expected[exp_idx ? exp_idx[slot] : slot]).
constexpr uint64_t kShaNotFinal = ~uint64_t(0);
// The kernel forms (ShaArgs::force, Knobs::sha_form).  4 and 5 were the
// same-round and one-message lag quad forms (removed; DESIGN_HISTORY.md).
enum ShaForm : int {
    kShaAuto = 0,     // by message count (launch_sha256)
    kShaOneWave = 1,  // one wave per 64 messages
    kShaSplit = 2,    // producer / consumer waves, one lane per message
    kShaStream = 3,   // persistent waves over (group, segment) items
    kShaLagPair = 6,  // two lanes per message, the a-side two rounds behind
};
struct ShaPiece {
    uint32_t* state = nullptr;        // [slots][8] (a..h); null: whole messages
    const uint32_t* slot = nullptr;   // [n]
    const uint64_t* total = nullptr;  // [n]
    uint32_t resume = 0;
};

struct ShaArgs {
    const uint8_t* const* ptrs;  // [n]
    const uint64_t* lens;        // [n]
    uint8_t* digests;            // [n][32] (may be null when only ok is wanted)
    const uint8_t* expected;     // [*][32] or null
    const uint64_t* exp_idx;     // [n]: message i compares expected[exp_idx[i]]
                                 //   (null: expected[i])
    uint8_t* ok;                 // [n] or null
    uint32_t n;
    int force = kShaAuto;        // a ShaForm (kShaStream needs the fields below)
    uint32_t n_cus = 0;          // the device's CUs (auto form choice; 0: 256)
    // Stream form (batches of more 64-message groups than the chip has
    // SIMDs): persistent waves take (group, segment) items in segment-major
    // order; a group's running state is handed from segment to segment
    // through `state`.  Every message 16-byte aligned.
    uint32_t* work = nullptr;    // [4 + groups] zeroed before the launch:
                                 //   [0] next item, [1] timeout code, [4 + g] segments of group g done
    uint32_t* state = nullptr;   // [n][8]
    uint32_t waves = 0;          // persistent waves
    uint32_t wg_waves = 1;       // waves per workgroup (1 or 4; waves divisible by it)
    uint32_t seg_max = 0;        // segments of the longest message
    ShaPiece piece;              // piece mode (kShaLagPair, or auto within its size)
};
// Messages per workgroup of the lag pair form (two consumer waves of 32, two
// lanes per message): the auto latency form, one workgroup per CU.
constexpr uint32_t kShaLagMsgs = 64;
// A chain's pace per 64-byte block on the MI355X (us), for host-side
// estimates of a launch's length (combiner.cpp): the lag pair form the auto
// choice takes up to kShaLagMsgs per CU (config 3: 19.1 ms for 16 384
// blocks, two producer waves since round 5), the split / one-wave forms
// beyond (29 ms per 1 MiB chunk).
constexpr double kShaLagUsPerBlock = 1.17;
constexpr double kShaSplitUsPerBlock = 1.8;
// Blocks per stream-form segment (32 KiB of each message).
constexpr uint32_t kShaSegBlocks = 512;
// Timeout code the stream form leaves in work[1] when a wave gave up
// waiting for a predecessor segment (the digests are then incomplete).
constexpr uint32_t kShaStreamTimeout = 0x5AA5u;

hipError_t launch_sha256(const ShaArgs& a, hipStream_t s);

// ---- PUT body digests (digest_kernel.hip) -----------------------------------
enum : uint32_t { kBodyMd5 = 0, kBodySha1 = 1, kBodySha256 = 2 };
struct BodyHashArgs {
    const uint8_t* const* ptrs;  // [n] device pointers
    const uint64_t* lens;        // [n]
    const uint32_t* algs;        // [gridDim.y] kBody* per launch row
    uint8_t* out;                // [n] records of out_stride bytes
    uint64_t out_stride;
    uint32_t off_md5, off_sha1, off_sha256;
    uint32_t n;
};
hipError_t launch_body_hash(const BodyHashArgs& a, uint32_t n_algs, hipStream_t s);

// A body's digests between two pieces (mxec_body_sums_update_device): one
// record of MXEC_SUMS_STATE_BYTES per body in the caller's HBM.  Every
// launch row owns its part: a chain per algorithm, each with its own tail (the
// three run side by side in one launch), and a running value per polynomial.
struct alignas(16) SumsChain {
    uint32_t h[8];      // chaining words (MD5 4, SHA-1 5, SHA-256 8)
    uint64_t bytes;     // hashed or pending so far; bytes % 64 are pending in tail
    uint64_t _pad;
    uint32_t tail[16];  // the unfinished block's bytes, in message order
};
struct SumsCrc {
    uint64_t bytes;  // covered by value
    uint32_t value;  // as crc32fast / crc32c_append hold it after those bytes
    uint32_t _pad;
};
struct alignas(16) SumsState {
    SumsChain chain[3];  // by kBody*
    SumsCrc crc[2];      // CRC32, CRC32C
};
static_assert(sizeof(SumsState) <= MXEC_SUMS_STATE_BYTES, "SumsState outgrew the caller's record");
constexpr uint32_t kSumsFirst = MXEC_SUMS_F_FIRST, kSumsFinal = MXEC_SUMS_F_FINAL;
// The update form: body i's piece continues state[i] (from the IV with
// kSumsFirst) and leaves its state there; with kSumsFinal it is padded with
// the total length and the digest goes to `out` as launch_body_hash writes it.
struct BodyHashUpdArgs {
    BodyHashArgs h;    // ptrs / lens: the pieces (a pointer may be null when its length is 0)
    uint8_t* state;    // [n] records of state_stride bytes (SumsState)
    uint64_t state_stride;
    uint32_t flags;    // kSums*
};
hipError_t launch_body_hash_update(const BodyHashUpdArgs& a, uint32_t n_algs, hipStream_t s);

// Per-polynomial constants (reflected domain), built on the host.
struct CrcTables {
    uint32_t poly;
    uint32_t slice[16][256];      // slice[k][b] = raw CRC of byte b followed by 15-k zero bytes
    uint32_t shift4k[4][256];     // byte k of v -> (v's byte k) * x^(8*4096)
    uint32_t shift_tile[4][256];  // same for x^(8*crc_tile_bytes())
    uint32_t lane_shift[256];     // x^(8*16*(255-L))
    uint32_t tile_pow[64];        // x^(8*TILE*2^j)
    uint32_t byte_pow[64];        // x^(8*2^j)
};
struct CrcBody {
    const uint8_t* base;   // floor16(p): 16-byte aligned
    const uint8_t* tail;   // last partial unit (tail_len < 16 bytes)
    uint64_t len;          // body length
    uint64_t tile0;        // first tile in the launch's tile space
    uint64_t n_tiles;
    uint64_t pad_units;    // leading virtual zero units of the first tile
    uint32_t head_skip;    // bytes of unit 0 before p
    uint32_t tail_len;
    uint32_t prev;         // running CRC to continue (crc32c_append); 0 = fresh
    uint32_t _pad;
};
struct CrcArgs {
    const CrcTables* tables;
    const CrcBody* bodies;  // [n_bodies], tile0 ascending
    const uint32_t* tile_body;  // [n_tiles] body of each tile
    uint32_t* tile_crc;     // [n_tiles] scratch
    uint8_t* out;           // finished CRC of body b at out + b * out_stride
    uint64_t out_stride;
    uint64_t n_tiles;
    uint32_t n_bodies;
};
uint64_t crc_tile_bytes();
hipError_t launch_crc(const CrcArgs& a, int n_cus, hipStream_t s);
// The update form of the finisher: the value to continue comes from
// state[body].crc[poly] instead of CrcBody::prev (0 with kSumsFirst) and the
// new running value goes back there; with kSumsFinal it also goes to a.out.
// The tile pass is launch_crc's: a piece's raw CRC does not depend on what
// came before it.
struct CrcCarry {
    uint8_t* state;  // [n_bodies] records of state_stride bytes (SumsState)
    uint64_t state_stride;
    uint32_t poly;   // 0 CRC32, 1 CRC32C
    uint32_t flags;  // kSums*
};
hipError_t launch_crc_update(const CrcArgs& a, const CrcCarry& c, int n_cus, hipStream_t s);

// ---- encrypt-then-EC frames (gcm_kernel.hip) ----------------------------------
// Per object (data key): AES-256 round keys as big-endian words, H^1..H^256
// and the 4-bit position table of H^256 (htab[p][v] = (v at nibble p) * H^256).
typedef uint32_t gcm_u32x4 __attribute__((ext_vector_type(4)));
struct GcmKey {
    uint32_t rk[60];
    gcm_u32x4 hpow[256];     // hpow[e - 1] = H^e
    gcm_u32x4 htab[32][16];
};
struct GcmFrame {
    const uint8_t* in;       // payload in (plaintext / ciphertext)
    union {
        uint8_t* out;        // payload out
        uint64_t ring_off;   // ring form: where the frame's plaintext starts in the ring (< ring_bytes)
    };
    union {
        uint8_t* hdr;        // encrypt: 12-byte nonce written here; decrypt: stored nonce
        uint64_t pos;        // window forms: the frame's byte offset in the frame stream, which is where
                             //   hdr, the stream side of in / out and tag are found; tag is unused, and
                             //   so is out (encrypt) or in (decrypt: out is the contiguous plaintext)
    };
    uint8_t* tag;            // encrypt: tag written here; decrypt: stored tag
    const uint8_t* aad;      // aad_len bytes (may be null when aad_len == 0)
    uint64_t index;          // chunk index of this frame
    uint32_t len;            // payload bytes (<= frame size)
    uint32_t aad_len;
    uint32_t key;            // index into keys
    uint32_t prefix_be;      // nonce prefix as a big-endian word (encrypt)
};
struct GcmArgs {
    const uint32_t* te;      // Te0..Te3, 4 x 256 words
    const GcmKey* keys;
    const GcmFrame* frames;  // frames of one object are consecutive
    int32_t* status;         // decrypt: 0 ok, 1 tag mismatch, 2 index mismatch
    uint64_t n_frames;
};
hipError_t launch_gcm_frames(const GcmArgs& a, bool decrypt, int n_cus, hipStream_t s);
// The forms whose frame stream lies in a ring of chunk slots: stream byte x
// is at base + ((x / chunk_size) % slots) * slot_stride + x % chunk_size.
// Encrypt writes the stream there from GcmFrame::in; decrypt reads it there,
// writes the plaintext to GcmFrame::out and the frame's status to status[f].
// Every frame's pos lies in [0, 2 * slots * chunk_size): the host rebases the
// launch by a multiple of slots * chunk_size (the mapping has that period), so
// a frame's slot is one division and one conditional subtract away.  A launch's
// frames span at most slots * chunk_size bytes and are shorter than 2^31.
struct GcmWinArgs : GcmArgs {
    uint8_t* base;
    uint64_t chunk_size, slot_stride, slots;
};
hipError_t launch_gcm_frames_window(const GcmWinArgs& a, bool decrypt, int n_cus, hipStream_t s);
// The decrypt form whose plaintext side is a byte ring: the frame stream is
// contiguous (GcmFrame::hdr / in / tag as in launch_gcm_frames), plaintext
// byte o of a frame is stored at ring + (ring_off + o) % ring_bytes, and the
// frame's status goes to status[f].  A frame is no longer than the ring, so at
// most one wrap cuts it; nothing outside [ring, ring + ring_bytes) and nothing
// in it outside the frames' ranges is written.
struct GcmRingArgs : GcmArgs {
    uint8_t* ring;
    uint64_t ring_bytes;
};
hipError_t launch_gcm_frames_ring(const GcmRingArgs& a, int n_cus, hipStream_t s);

// ---- host <-> device copies by CU waves (copy_kernel.hip) ---------------------
// One block of a copy batch: len bytes from src to dst (one side host memory
// mapped into the GPU's address space, the other HBM).  The table itself may
// sit in mapped host memory.
struct alignas(16) CopyBlk {
    uint64_t dst, src, len, pad;
};
constexpr uint64_t kCopyBlock = uint64_t(256) << 10;  // bytes per block (at most)
hipError_t launch_copy_blocks(const CopyBlk* blks, uint64_t n, bool to_host, uint32_t grid, hipStream_t s);
// Whether a host <-> device segment suits the wave copy: both ends at the
// same offset modulo 16 (then only its head and tail bytes go bytewise).
inline bool copy_phase_ok(const void* host, const void* dev) {
    return ((reinterpret_cast<uintptr_t>(host) ^ reinterpret_cast<uintptr_t>(dev)) & 15) == 0;
}

}  // namespace mxec
