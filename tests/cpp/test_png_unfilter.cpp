// test_png_unfilter.cpp -- the schedule of the PNG reconstruction kernel (zlibstream_amd/csrc/zs_png.hip, KU) run on the host
// with the code the kernel compiles (zs_png.h): the scan that validates the type bytes and cuts an image into segments, and
// for every segment the waves of a workgroup advancing in chunk steps -- 64 skewed lanes per wave, a ring of two tile
// columns per wave, the boundary row handed from a band to the next through a two-slot buffer or, where the bands wrap
// around the waves, read back from the output.  Compared with a plain row-by-row reconstruction (PNG specification 9.2).
// Anything the schedule reads before it was produced shows as a difference: the model's buffers start poisoned.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_png.h"

using namespace zs;

namespace {

struct Seg {
    int row0, row1;
};

// the plain definition, written independently of zs_png.h
void reference(const std::vector<uint8_t> &in, int64_t rb, int h, int bpp, std::vector<uint8_t> &out) {
    out.assign((size_t)(rb * h), 0);
    for (int y = 0; y < h; y++) {
        const uint8_t *f = &in[(size_t)y * (size_t)(rb + 1)];
        const int ft = f[0];
        for (int64_t i = 0; i < rb; i++) {
            const int a = i >= bpp ? out[(size_t)(y * rb + i - bpp)] : 0;
            const int b = y > 0 ? out[(size_t)((y - 1) * rb + i)] : 0;
            const int c = (y > 0 && i >= bpp) ? out[(size_t)((y - 1) * rb + i - bpp)] : 0;
            int pr = 0;
            if (ft == 1) pr = a;
            else if (ft == 2) pr = b;
            else if (ft == 3) pr = (a + b) / 2;
            else if (ft == 4) {
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
            }
            out[(size_t)(y * rb + i)] = (uint8_t)(f[1 + i] + pr);
        }
    }
}

// the scan kernel: first row with a type above 4, and the segments
int scan(const std::vector<uint8_t> &in, int64_t rb, int h, std::vector<Seg> &segs) {
    int bad = -1;
    segs.clear();
    for (int r = 0; r < h; r++) {
        const int ft = in[(size_t)r * (size_t)(rb + 1)];
        if (ft > 4 && bad < 0) bad = r;
        if (r == 0 || png_row_cuts(ft)) {
            if (!segs.empty()) segs.back().row1 = r;
            segs.push_back(Seg{r, h});
        }
    }
    return bad;
}

template <int BPP>
uint64_t get_px(const uint8_t *p) {
    uint64_t v = 0;
    for (int j = 0; j < BPP; j++) v |= (uint64_t)p[j] << (8 * j);
    return v;
}
template <int BPP>
void put_px(uint8_t *p, uint64_t v) {
    for (int j = 0; j < BPP; j++) p[j] = (uint8_t)(v >> (8 * j));
}

struct Wave {
    int64_t k, q;
    uint64_t a[64], cprev[64], pout[64];
    PngSel sel[64];
    bool rowvalid[64];
};

// png_segment of zs_png.hip, phase by phase
template <int BPP>
void segment(const uint8_t *in, uint8_t *out, int64_t rb, int row0, int row1, int waves) {
    const int stride = png_tile_stride(BPP), col_bytes = kPngChunk * BPP;
    static std::vector<uint8_t> lds;  // (what an earlier segment left in it is as good a poison as any)
    if (lds.size() < (size_t)png_lds_bytes(BPP, waves)) lds.assign((size_t)png_lds_bytes(BPP, waves), 0xA5);
    const int bnd_off = waves * kPngRows * stride;
    const int64_t npx = png_npx(rb, BPP), nq = png_nq(npx);
    const int64_t nbands = ((int64_t)(row1 - row0) + kPngRows - 1) / kPngRows;
    const int64_t steps = png_total_steps(nbands, waves, nq), period = png_period(nq, waves);
    std::vector<Wave> wv((size_t)waves);
    for (int w = 0; w < waves; w++) wv[(size_t)w].k = w, wv[(size_t)w].q = -2 * (int64_t)w;
    std::vector<int64_t> done((size_t)nbands, 0);
    for (int64_t T = 0; T < steps; T++) {
        // two barriers per chunk step: every wave has taken its tile column in before any reconstructs, and every wave has
        // stored and handed on before any takes in the next (stage 0: loads; stages 1 and 2 of a wave follow each other)
        for (int stage = 0; stage < 2; stage++)
            for (int w = 0; w < waves; w++)
              for (int phase = stage; phase <= 2 * stage; phase++) {
                Wave &W = wv[(size_t)w];
                const int64_t k = W.k, q = W.q;
                const bool active = q >= 0 && q < nq && k < nbands;
                if (!active) continue;
                if (q != T - png_band_off(k, waves, nq)) {
                    printf("FAIL: wave %d at step %lld is not where png_band_off puts band %lld\n", w, (long long)T, (long long)k);
                    exit(1);
                }
                uint8_t *tile = &lds[(size_t)(w * kPngRows * stride)], *bnd = &lds[(size_t)(bnd_off + w * kPngBndBytes)];
                const int64_t y0 = row0 + k * kPngRows;
                const int rows = (int)((int64_t)row1 - y0 < kPngRows ? (int64_t)row1 - y0 : kPngRows);
                const int slot = (int)(q & 1);
                if (phase == 0) {
                    if (q == 0)
                        for (int L = 0; L < 64; L++) {
                            W.a[L] = W.cprev[L] = W.pout[L] = 0;
                            W.rowvalid[L] = L < rows;
                            W.sel[L] = png_sel(W.rowvalid[L] ? in[(size_t)((y0 + L) * (rb + 1))] : 0);
                        }
                    const int64_t byte0 = q * col_bytes;
                    const int nbytes = (int)(rb - byte0 < col_bytes ? rb - byte0 : col_bytes);
                    if (nbytes > 0) {
                        for (int i = 0; i < rows; i++)
                            memcpy(tile + i * stride + slot * col_bytes, in + (y0 + i) * (rb + 1) + 1 + byte0, (size_t)nbytes);
                        if (w == 0) {
                            if (k == 0) memset(bnd + slot * col_bytes, 0, (size_t)col_bytes);
                            else memcpy(bnd + slot * col_bytes, out + (y0 - 1) * rb + byte0, (size_t)nbytes);
                        }
                    }
                } else if (phase == 1) {
                    const uint8_t *bcol = bnd + slot * col_bytes;
                    for (int s = 0; s < kPngChunk; s++) {
                        uint64_t prev[64];  // the lanes step together: the shift reads what every lane held before this step
                        memcpy(prev, W.pout, sizeof prev);
                        for (int L = 0; L < rows; L++) {  // (a lane without a row produces zeros that no lane with a row reads)
                            const int64_t x = q * kPngChunk + s - L;
                            const bool act = W.rowvalid[L] && x >= 0 && x < npx;
                            uint8_t *p = tile + L * stride + (int)(x & (kPngRing - 1)) * BPP;
                            const uint64_t f = act ? get_px<BPP>(p) : 0;
                            const uint64_t b = L > 0 ? prev[L - 1] : get_px<BPP>(bcol + s * BPP);
                            const uint64_t rec = png_recon_px<BPP>(W.sel[L], f, W.a[L], b, W.cprev[L]);
                            W.pout[L] = act ? rec : 0;
                            W.a[L] = act ? rec : W.a[L];
                            W.cprev[L] = b;
                            if (act) put_px<BPP>(p, rec);
                        }
                    }
                } else {
                    if (q >= 1) {
                        const int64_t byte0 = (q - 1) * col_bytes;
                        const int nbytes = (int)(rb - byte0 < col_bytes ? rb - byte0 : col_bytes);
                        const int pslot = slot ^ 1;
                        for (int i = 0; i < rows; i++) memcpy(out + (y0 + i) * rb + byte0, tile + i * stride + pslot * col_bytes, (size_t)nbytes);
                        if (w + 1 < waves)
                            memcpy(bnd + kPngBndBytes + pslot * col_bytes, tile + (kPngRows - 1) * stride + pslot * col_bytes, (size_t)col_bytes);
                    }
                    if (q == nq - 1) done[(size_t)k]++;
                }
            }
        for (int w = 0; w < waves; w++)
            if (++wv[(size_t)w].q == period) wv[(size_t)w].q = 0, wv[(size_t)w].k += waves;
    }
    for (int64_t k = 0; k < nbands; k++)
        if (done[(size_t)k] != 1) {
            printf("FAIL: band %lld of %lld ran to its end %lld times\n", (long long)k, (long long)nbands, (long long)done[(size_t)k]);
            exit(1);
        }
}

void segment_any(int bpp, const uint8_t *in, uint8_t *out, int64_t rb, int row0, int row1, int waves) {
    switch (bpp) {
    case 1: segment<1>(in, out, rb, row0, row1, waves); break;
    case 2: segment<2>(in, out, rb, row0, row1, waves); break;
    case 3: segment<3>(in, out, rb, row0, row1, waves); break;
    case 4: segment<4>(in, out, rb, row0, row1, waves); break;
    case 5: segment<5>(in, out, rb, row0, row1, waves); break;
    case 6: segment<6>(in, out, rb, row0, row1, waves); break;
    case 7: segment<7>(in, out, rb, row0, row1, waves); break;
    default: segment<8>(in, out, rb, row0, row1, waves); break;
    }
}

std::mt19937 rng(20250917);
long n_cases = 0, n_segments = 0;

// mode 0..4: that type in every row; 5: a random valid type per row; 6: mostly Up/Average/Paeth with a cut now and then
void run_case(int bpp, int64_t rb, int h, int mode, int waves) {
    std::vector<uint8_t> in((size_t)((rb + 1) * h));
    for (auto &v : in) v = (uint8_t)rng();
    for (int y = 0; y < h; y++) {
        int ft = mode;
        if (mode == 5) ft = (int)(rng() % 5);
        if (mode == 6) ft = rng() % 97 == 0 ? (int)(rng() % 2) : 2 + (int)(rng() % 3);
        in[(size_t)y * (size_t)(rb + 1)] = (uint8_t)ft;
    }
    std::vector<uint8_t> want, got((size_t)(rb * h), 0x5A);
    reference(in, rb, h, bpp, want);
    std::vector<Seg> segs;
    if (scan(in, rb, h, segs) >= 0) {
        printf("FAIL: the scan reports a bad row in a valid image\n");
        exit(1);
    }
    // the cut rule: a segment starts at row 0 and at every None / Sub row, and nowhere else
    size_t si = 0;
    for (int y = 0; y < h; y++) {
        const int ft = in[(size_t)y * (size_t)(rb + 1)];
        const bool starts = y == 0 || ft == 0 || ft == 1;
        if (starts != (si < segs.size() && segs[si].row0 == y)) {
            printf("FAIL: cut rule at row %d\n", y);
            exit(1);
        }
        if (starts) si++;
    }
    // the segments share nothing: run them last to first
    for (size_t i = segs.size(); i-- > 0;) segment_any(bpp, in.data(), got.data(), rb, segs[i].row0, segs[i].row1, waves);
    if (got != want) {
        size_t d = 0;
        while (got[d] == want[d]) d++;
        printf("FAIL: bpp %d row_bytes %lld height %d mode %d waves %d: first difference at row %lld byte %lld\n", bpp, (long long)rb, h, mode, waves,
               (long long)(d / (size_t)rb), (long long)(d % (size_t)rb));
        exit(1);
    }
    n_cases++;
    n_segments += (long)segs.size();
}

}  // namespace

int main() {
    const int heights[] = {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049};
    for (int bpp = 1; bpp <= 8; bpp++) {
        const int64_t rbs[] = {1, bpp - 1, bpp, bpp + 1, 63, 64, 65, 1000, 4097};
        for (int64_t rb : rbs) {
            if (rb < 1) continue;  // (bpp - 1 of bpp 1)
            for (int h : heights)
                for (int mode = 0; mode <= 6; mode++) run_case(bpp, rb, h, mode, png_waves(bpp));
        }
        // other workgroup sizes: one wave (every band wraps), three, and more waves than a short row has chunk steps
        for (int waves : {1, 3, 8})
            for (int64_t rb : {(int64_t)bpp, (int64_t)65, (int64_t)(200 * bpp + 1)})
                for (int h : {1, 64, 65, 700})
                    for (int mode : {3, 4, 5, 6}) run_case(bpp, rb, h, mode, waves);
    }
    // the bad-type scan: the first row with a type above 4 is the one reported, and such a row cuts
    for (int t = 0; t < 200; t++) {
        const int h = 1 + (int)(rng() % 300), rb = 1 + (int)(rng() % 40);
        std::vector<uint8_t> in((size_t)((rb + 1) * h), 0);
        for (int y = 0; y < h; y++) in[(size_t)(y * (rb + 1))] = (uint8_t)(rng() % 5);
        int first = -1;
        for (int j = 0, nbad = (int)(rng() % 4); j < nbad; j++) {
            const int y = (int)(rng() % (unsigned)h);
            in[(size_t)(y * (rb + 1))] = (uint8_t)(5 + rng() % 251);
            if (first < 0 || y < first) first = y;
        }
        std::vector<Seg> segs;
        if (scan(in, rb, h, segs) != first) {
            printf("FAIL: bad-type scan\n");
            return 1;
        }
        for (const Seg &s : segs)
            if (s.row0 >= s.row1) {
                printf("FAIL: empty segment\n");
                return 1;
            }
    }
    printf("PASS %ld images, %ld segments\n", n_cases, n_segments);
    return 0;
}
