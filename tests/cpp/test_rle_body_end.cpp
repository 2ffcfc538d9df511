// rle_body_end and rle_refills_fired_at of zs_rle.h on the host: reads "n kl" lines (decimal), prints "H k_done" for each, k_done
// the refills fired at H.  tests/test_rle_cases.py compares them with the hand-over positions the catalogue's issue names.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../../zlibstream_amd/csrc/zs_rle.h"

int main() {
    int64_t n;
    int kl;
    while (scanf("%" SCNd64 " %d", &n, &kl) == 2) {
        const int64_t h = zs::rle_body_end(n);
        printf("%" PRId64 " %d\n", h, h < 0 ? 0 : zs::rle_refills_fired_at(h, kl));
    }
    return 0;
}
