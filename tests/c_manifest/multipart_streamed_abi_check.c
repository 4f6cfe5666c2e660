/* multipart_streamed_abi_check.c -- the streaming CompleteMultipartUpload's
 * declarations compile as C and resolve in libmaxio_ec.so
 * (tests/test_multipart_streamed_abi.py builds and runs it against the built
 * library).  Nothing is launched: the calls made are those whose arguments
 * are refused before a context or a device is looked at. */
#include <stdio.h>
#include <string.h>

#include "../../include/maxio_ec.h"

typedef int (*ring_fn)(mxec_ctx*, int, void*, const mxec_frames_job*, uint64_t, const uint64_t*, const void*, int32_t*);
typedef int (*plain_fn)(mxec_ctx*, const char*, uint64_t, uint32_t, const mxec_multipart_part*, uint32_t, uint64_t,
                        char[48]);
typedef int (*enc_fn)(mxec_ctx*, const char*, uint64_t, uint32_t, const mxec_multipart_part*, uint32_t,
                      const uint8_t[32], const char*, const uint8_t[32], const uint8_t[4], const uint8_t*, uint32_t,
                      uint64_t, char[48]);

int main(void) {
    ring_fn ring_call = mxec_frames_decrypt_ring_device;
    plain_fn plain_call = mxec_complete_multipart_streamed;
    enc_fn enc_call = mxec_complete_multipart_streamed_encrypted;
    struct mxec_frames_ring r1;
    mxec_frames_ring r2;
    char etag[48];
    uint8_t key[32] = {0}, prefix[4] = {0};
    uint64_t off = 0;
    mxec_frames_job job;
    mxec_multipart_part part;
    memset(&job, 0, sizeof job);
    memset(&part, 0, sizeof part);
    r1.base_dev = 0;
    r1.bytes = 0;
    r2 = r1;
    if (sizeof(mxec_frames_ring) != 16 || sizeof r1 != sizeof r2) return 1;
    /* nothing to do */
    if (ring_call(0, 0, 0, 0, 0, 0, 0, 0) != MXEC_OK) return 2;
    /* a null ring base */
    job.key = key;
    job.frame_size = 64;
    if (ring_call(0, 0, 0, &job, 1, &off, &r2, 0) != MXEC_E_INVALID_ARG) return 3;
    if (!strstr(mxec_last_error(), "null argument")) return 4;
    /* null arguments, and an encrypted part given to the plain call */
    if (plain_call(0, "x.ec", 4096, 2, 0, 1, 0, etag) != MXEC_E_INVALID_ARG) return 5;
    part.path = "part";
    part.encrypted = 1;
    if (plain_call(0, "x.ec", 4096, 2, &part, 1, 0, etag) != MXEC_E_INVALID_ARG) return 6;
    if (!strstr(mxec_last_error(), "encrypted part")) return 7;
    if (enc_call(0, "x.ec", 4096, 2, &part, 1, key, "id", 0, prefix, 0, 0, 0, etag) != MXEC_E_INVALID_ARG) return 8;
    puts("multipart_streamed abi ok");
    return 0;
}
