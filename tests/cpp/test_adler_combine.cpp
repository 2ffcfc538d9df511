// adler_combine of zs_core.h on the host: reads "a1 a2 len2" lines (decimal), prints the combined Adler-32 of each.
// tests/test_match_cases.py compares them with zlib.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../../zlibstream_amd/csrc/zs_core.h"

int main() {
    uint64_t a1, a2, len2;
    while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a1, &a2, &len2) == 3) printf("%u\n", zs::adler_combine((uint32_t)a1, (uint32_t)a2, len2));
    return 0;
}
