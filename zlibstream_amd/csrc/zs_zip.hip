// zs_zip.hip -- the one kernel of the ZIP container (zs_zip.h holds the rules): KZ, the closing kernel behind the framing
// launch of zs_zip_encode_batch_device (KC, zs_crc32.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "zs_zip.h"

namespace zs {

// An entry's CRC-32 as KC's finishing launch left it in crc[span], little-endian into the two places that carry it: the
// local header and the central record, both of any alignment, so byte by byte.  One lane per entry; with it an archive is
// finished without the CRCs going to the host and back.
__global__ __launch_bounds__(64) void zs_zip_close_kernel(const ZipClose *__restrict__ closes, int n, const uint32_t *__restrict__ crc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ZipClose z = closes[i];
    const uint32_t v = crc[z.span];
    for (int k = 0; k < 4; k++) z.local_crc[k] = (uint8_t)(v >> (8 * k)), z.central_crc[k] = (uint8_t)(v >> (8 * k));
}

}  // namespace zs
