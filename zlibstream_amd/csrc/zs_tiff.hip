// zs_tiff.hip -- KT, the two predictor kernels of the TIFF calls (zs_tiff.h holds the container's rules and the per-lane step):
//   zs_tiff_undo_kernel     decoded chunks -> the row-major image: the horizontal predictor (2) or the floating-point
//                           predictor (3) undone, big-endian samples swapped, a tile clipped at the image's edges
//   zs_tiff_predict_kernel  the inverse: strips and tiles cut from the image, a tile's surplus padded by repetition,
//                           differenced (2) or split into byte planes and differenced (3)
// Both run over the flat list of all chunk rows of a call, one wave per row, a row of any length in passes of 64 lanes x
// 16 bytes.  A lane's group is bytes [16 g, 16 g + 16) of the row -- whole samples whatever the row's address is, read and
// written with one 16-byte access (global memory takes them at any alignment); the group that a row ends in goes byte by
// byte.  No atomics, no LDS, and every output byte has one writer.
#pragma once

#include <hip/hip_runtime.h>

#include "zs_png.h"
#include "zs_tiff.h"

namespace zs {

typedef uint32_t tiff_u32x4 __attribute__((ext_vector_type(4)));
typedef tiff_u32x4 tiff_u32x4_a1 __attribute__((aligned(1)));  // 16 bytes at any address: one global_load_dwordx4 / global_store_dwordx4
typedef uint32_t tiff_u32_a1 __attribute__((aligned(1)));
typedef uint16_t tiff_u16_a1 __attribute__((aligned(1)));

constexpr int kTiffRowsPerWg = 4;
constexpr int kTiffPass = 64 * 16;  // bytes of a row that one pass of the wave takes

// bytes [off, off + 16) of a row of n bytes at p, as four little-endian words; what lies behind the row reads as zero
__device__ __forceinline__ void tiff_load_group(const uint8_t *p, int off, int n, uint32_t w[4]) {
    w[0] = w[1] = w[2] = w[3] = 0;
    if (off + 16 <= n) {
        const tiff_u32x4 v = *(const tiff_u32x4_a1 *)(p + off);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else {
        for (int b = off; b < n; b++) w[(b - off) >> 2] |= (uint32_t)p[b] << (8 * ((b - off) & 3));
    }
}
// ... and the store: only bytes in front of n
__device__ __forceinline__ void tiff_store_group(uint8_t *p, int off, int n, const uint32_t w[4]) {
    if (off + 16 <= n) {
        tiff_u32x4 v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        *(tiff_u32x4_a1 *)(p + off) = v;
    } else {
        for (int b = off; b < n; b++) p[b] = (uint8_t)(w[(b - off) >> 2] >> (8 * ((b - off) & 3)));
    }
}

// the sum of x over lanes 0 .. lane (ds_bpermute steps)
__device__ __forceinline__ uint32_t tiff_wave_scan(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)x, d, 64);
        x += lane >= d ? t : 0;
    }
    return x;
}
__device__ __forceinline__ uint32_t tiff_wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}

// One pass of the stride-SPP prefix sum over the wave's 64 groups: v (this lane's samples, its phase p0) become the sums
// of the row up to them, given carry[c] = the row's sum of channel c in front of the pass, which is moved on.
template <int E, int SPP>
__device__ __forceinline__ void tiff_wave_pass(uint32_t *v, int p0, uint32_t *carry, int lane) {
    uint32_t tot[SPP], add[SPP];
    tiff_lane_scan<E, SPP>(v, p0, tot);
#pragma unroll
    for (int c = 0; c < SPP; c++) {
        const uint32_t upto = tiff_wave_scan(tot[c], lane);
        add[c] = carry[c] + upto - tot[c];
        carry[c] += (uint32_t)__builtin_amdgcn_readlane((int)upto, 63);
    }
    tiff_lane_add<E, SPP>(v, p0, add);
}

// predictor 2 undone: nb bytes of samples are summed, the first cb of them stored
template <int S, int SPP>
__device__ void tiff_undo_row(const uint8_t *src, uint8_t *dst, int nb, int cb, bool swap, int lane) {
    constexpr int E = 16 / S;
    uint32_t carry[SPP];
#pragma unroll
    for (int c = 0; c < SPP; c++) carry[c] = 0;
    for (int base = 0; base < cb; base += kTiffPass) {  // (what lies behind cb is read by nobody: a sum looks to the left only)
        const int off = base + 16 * lane;
        uint32_t w[4], v[E];
        tiff_load_group(src, off, nb, w);
        tiff_unpack<S>(w, v, swap);
        tiff_wave_pass<E, SPP>(v, tiff_phase<E, SPP>(off >> 4), carry, lane);
        tiff_pack<S>(v, w);
        tiff_store_group(dst, off, cb, w);
    }
}

// predictor 1: a copy, big-endian samples swapped
template <int S>
__device__ void tiff_copy_row(const uint8_t *src, uint8_t *dst, int cb, bool swap, int lane) {
    constexpr int E = 16 / S;
    for (int base = 0; base < cb; base += kTiffPass) {
        const int off = base + 16 * lane;
        uint32_t w[4], v[E];
        tiff_load_group(src, off, cb, w);
        if (S > 1 && swap) {
            tiff_unpack<S>(w, v, true);
            tiff_pack<S>(v, w);
        }
        tiff_store_group(dst, off, cb, w);
    }
}

// predictor 3 undone.  The row is four planes of N = nb / 4 bytes, plane k holding byte k of every sample, the most
// significant first; the byte-wise sum with stride SPP runs through all 4 N bytes, so plane k begins with what the planes in
// front of it hold of each channel (N is a multiple of SPP: byte k N + j has the channel of byte j).  First those sums,
// then sixteen samples a lane: one group of each plane, summed with the plane's own carry, gathered into little-endian words.
template <int SPP>
__device__ void tiff_undo_float_row(const uint8_t *src, uint8_t *dst, int nb, int cb, int lane) {
    const int N = nb >> 2, n_out = cb >> 2;
    uint32_t carry[4][SPP];
#pragma unroll
    for (int c = 0; c < SPP; c++) carry[0][c] = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t sum[SPP];
#pragma unroll
        for (int c = 0; c < SPP; c++) sum[c] = 0;
        for (int base = 0; base < N; base += kTiffPass) {
            const int off = base + 16 * lane;
            uint32_t w[4], v[16], tot[SPP];
            tiff_load_group(src + (int64_t)k * N, off, N, w);
            tiff_unpack<1>(w, v, false);
            tiff_lane_scan<16, SPP>(v, tiff_phase<16, SPP>(off >> 4), tot);
#pragma unroll
            for (int c = 0; c < SPP; c++) sum[c] += tot[c];
        }
#pragma unroll
        for (int c = 0; c < SPP; c++) carry[k + 1][c] = carry[k][c] + tiff_wave_sum(sum[c]);
    }
    for (int base = 0; base < n_out; base += kTiffPass) {
        const int off = base + 16 * lane;  // the lane's first sample
        const int p0 = tiff_phase<16, SPP>(off >> 4);
        uint32_t px[16];
#pragma unroll
        for (int j = 0; j < 16; j++) px[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t w[4], v[16];
            tiff_load_group(src + (int64_t)k * N, off, N, w);
            tiff_unpack<1>(w, v, false);
            tiff_wave_pass<16, SPP>(v, p0, carry[k], lane);
#pragma unroll
            for (int j = 0; j < 16; j++) px[j] |= (v[j] & 0xFF) << (8 * (3 - k));
        }
#pragma unroll
        for (int q = 0; q < 4; q++) tiff_store_group(dst, 4 * off + 16 * q, cb, px + 4 * q);
    }
}

template <int SPP>
__device__ void tiff_undo_spp(const TiffJob &jb, const uint8_t *src, uint8_t *dst, int lane) {
    if (jb.predictor == 3) tiff_undo_float_row<SPP>(src, dst, jb.nb, jb.cb, lane);
    else if (jb.sample_bytes == 1) tiff_undo_row<1, SPP>(src, dst, jb.nb, jb.cb, false, lane);
    else if (jb.sample_bytes == 2) tiff_undo_row<2, SPP>(src, dst, jb.nb, jb.cb, jb.swap != 0, lane);
    else tiff_undo_row<4, SPP>(src, dst, jb.nb, jb.cb, jb.swap != 0, lane);
}

// the flat row `first + (this wave's place in the grid)` of the launch: its job and its row there, false behind the list
__device__ __forceinline__ bool tiff_my_row(const int32_t *row_off, int n, int64_t first, int *job, int *r) {
    const int64_t row = first + (int64_t)blockIdx.x * kTiffRowsPerWg + (threadIdx.x >> 6);
    if (row >= row_off[n]) return false;
    *job = png_row_image(row_off, n, row);
    *r = (int)(row - row_off[*job]);
    return true;
}

__global__ __launch_bounds__(64 * kTiffRowsPerWg) void zs_tiff_undo_kernel(const TiffJob *__restrict__ jobs, const int32_t *__restrict__ row_off, int n, int64_t first) {
    int j, r;
    if (!tiff_my_row(row_off, n, first, &j, &r)) return;
    const TiffJob jb = jobs[j];
    const int lane = (int)threadIdx.x & 63;
    const uint8_t *src = jb.chunk + (int64_t)r * jb.chunk_pitch;
    uint8_t *dst = jb.image + (int64_t)r * jb.image_pitch;
    if (jb.predictor == 1) {
        if (jb.sample_bytes == 2) tiff_copy_row<2>(src, dst, jb.cb, jb.swap != 0, lane);
        else if (jb.sample_bytes == 4) tiff_copy_row<4>(src, dst, jb.cb, jb.swap != 0, lane);
        else tiff_copy_row<1>(src, dst, jb.cb, false, lane);
        return;
    }
    switch (jb.spp) {  // (the same for the whole wave)
    case 1: tiff_undo_spp<1>(jb, src, dst, lane); break;
    case 2: tiff_undo_spp<2>(jb, src, dst, lane); break;
    case 3: tiff_undo_spp<3>(jb, src, dst, lane); break;
    case 4: tiff_undo_spp<4>(jb, src, dst, lane); break;
    case 5: tiff_undo_spp<5>(jb, src, dst, lane); break;
    case 6: tiff_undo_spp<6>(jb, src, dst, lane); break;
    case 7: tiff_undo_spp<7>(jb, src, dst, lane); break;
    default: tiff_undo_spp<8>(jb, src, dst, lane); break;
    }
}

// ---- the forward kernel.  Every output sample is the difference of two input samples, so there is no sum to carry: a lane
// fetches its group's samples one by one (its neighbours' fetches hit the same lines) and stores the group in one piece.
template <int S>
__device__ __forceinline__ uint32_t tiff_sample(const uint8_t *p, int s) {
    if constexpr (S == 1) return p[s];
    else if constexpr (S == 2) return *(const tiff_u16_a1 *)(p + 2 * s);
    else return *(const tiff_u32_a1 *)(p + 4 * s);
}

// row samples [0, ns) of which the first ns_in lie in the image; sample s behind them is the last pixel's of its channel
template <int S>
__device__ void tiff_predict_row(const uint8_t *src, uint8_t *dst, int nb, int cb, int spp, bool diff, int lane) {
    constexpr int E = 16 / S;
    const int ns = nb / S, ns_in = cb / S, last_px = ns_in - spp;
    for (int base = 0; base < nb; base += kTiffPass) {
        const int off = base + 16 * lane, s0 = off / S;
        int ch = s0 % spp;
        uint32_t v[E], w[4];
#pragma unroll
        for (int j = 0; j < E; j++) {
            const int s = s0 + j;
            v[j] = 0;
            if (s < ns) {
                const uint32_t x = tiff_sample<S>(src, s < ns_in ? s : last_px + ch);
                const int sp = s - spp;
                const uint32_t left = diff && sp >= 0 ? tiff_sample<S>(src, sp < ns_in ? sp : last_px + ch) : 0;
                v[j] = x - left;
            }
            ch = ch + 1 == spp ? 0 : ch + 1;
        }
        tiff_pack<S>(v, w);
        tiff_store_group(dst, off, nb, w);
    }
}

// byte b of the plane-split row: plane k = b / N holds byte 3 - k of the little-endian float j = b mod N
__device__ __forceinline__ uint32_t tiff_plane_byte(const uint8_t *src, int k, int j, int n_in, int spp) {
    const int s = j < n_in ? j : n_in - spp + j % spp;
    return src[4 * s + (3 - k)];
}
__device__ void tiff_predict_float_row(const uint8_t *src, uint8_t *dst, int nb, int cb, int spp, int lane) {
    const int N = nb >> 2, n_in = cb >> 2;
    for (int base = 0; base < nb; base += kTiffPass) {
        const int off = base + 16 * lane;
        uint32_t w[4] = {0, 0, 0, 0};
        int k = off / N, j = off - k * N;
        for (int i = 0; i < 16 && off + i < nb; i++) {
            int kl = k, jl = j - spp;  // the byte spp in front, which may lie in the plane before
            if (jl < 0) kl--, jl += N;
            const uint32_t x = tiff_plane_byte(src, k, j, n_in, spp), left = kl >= 0 ? tiff_plane_byte(src, kl, jl, n_in, spp) : 0;
            w[i >> 2] |= ((x - left) & 0xFF) << (8 * (i & 3));
            if (++j == N) j = 0, k++;
        }
        tiff_store_group(dst, off, nb, w);
    }
}

__global__ __launch_bounds__(64 * kTiffRowsPerWg) void zs_tiff_predict_kernel(const TiffJob *__restrict__ jobs, const int32_t *__restrict__ row_off, int n, int64_t first) {
    int j, r;
    if (!tiff_my_row(row_off, n, first, &j, &r)) return;
    const TiffJob jb = jobs[j];
    const int lane = (int)threadIdx.x & 63;
    const int rr = r < jb.rows_in ? r : jb.rows_in - 1;  // a tile's rows below the image repeat its last row
    const uint8_t *src = jb.image + (int64_t)rr * jb.image_pitch;
    uint8_t *dst = jb.chunk + (int64_t)r * jb.chunk_pitch;
    if (jb.predictor == 3) tiff_predict_float_row(src, dst, jb.nb, jb.cb, jb.spp, lane);
    else if (jb.sample_bytes == 1) tiff_predict_row<1>(src, dst, jb.nb, jb.cb, jb.spp, jb.predictor == 2, lane);
    else if (jb.sample_bytes == 2) tiff_predict_row<2>(src, dst, jb.nb, jb.cb, jb.spp, jb.predictor == 2, lane);
    else tiff_predict_row<4>(src, dst, jb.nb, jb.cb, jb.spp, jb.predictor == 2, lane);
}

}  // namespace zs
