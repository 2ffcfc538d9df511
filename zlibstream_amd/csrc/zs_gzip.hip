// zs_gzip.hip -- the two small kernels of the gzip container (zs_gzip.h holds the rules): the header kernel in front of an
// inflate call, one lane per member, and the trailer kernel behind a deflate call's framing launch (KC, zs_crc32.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "zs_gzip.h"

namespace zs {

struct GzMember {
    const uint8_t *in;
    int64_t in_len;
};
// what the header kernel leaves per member: 16 bytes, one store
struct GzHead {
    int32_t body_off;     // where the deflate body begins
    int32_t member_size;  // BGZF: BSIZE + 1; 0: no BGZF subfield
    int32_t err;          // GzErr
    int32_t pad_;
};
static_assert(sizeof(GzHead) == 16, "one 16-byte store per member");

__global__ __launch_bounds__(64) void zs_gzip_header_kernel(const GzMember *__restrict__ members, int n, GzHead *__restrict__ heads) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GzMember m = members[i];
    GzHeader h;
    const int err = gzip_parse_header(m.in, m.in_len, &h);
    *(int4 *)(heads + i) = make_int4((int)h.body_off, (int)h.member_size, err, 0);
}

// A gzip member's trailer behind its framed body: the CRC-32 of the input as KC's finishing launch left it in crc[crc_idx],
// then the input's length mod 2^32, both little-endian, at a destination of any alignment.
struct GzTrail {
    uint8_t *dst;
    uint32_t crc_idx, isize;
};
__global__ __launch_bounds__(64) void zs_gzip_trailer_kernel(const GzTrail *__restrict__ trails, int n, const uint32_t *__restrict__ crc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const GzTrail t = trails[i];
    const uint32_t v = crc[t.crc_idx];
    for (int k = 0; k < 4; k++) t.dst[k] = (uint8_t)(v >> (8 * k)), t.dst[4 + k] = (uint8_t)(t.isize >> (8 * k));
}

}  // namespace zs
