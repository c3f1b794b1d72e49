// media_amd/csrc/k_dec_out_scale.h -- decoder output at a requested size: the pictures of a call area-resampled out of the
// reconstruction ring into the packed destination of k_dec_out.h, in ONE launch (include/mi355x_h264_dec.h, "output size").
//
// The arithmetic is the one of scaled streams (include/mi355x_h264.h; scale_kernels.h holds its device form, which is used here and
// not stated again: ScaleDiv, scale_divide, scale_taps).  The delivered picture is what k_dec_out delivers for a picture whose
// cropped planes are the resampled ones: Y from (w, h) to (W, H), Cb and Cr from (w / 2, h / 2) to (W / 2, H / 2); RGBA converts
// the RESULT, the chroma sample of a 2x2 block of it serving its four pixels.  A position whose result size is its source size goes
// through ratio 1 (one tap of weight s per axis, N = D v) and gives k_dec_out's bytes.
//
// blockIdx.z = position.  tab[position] (DecOutScalePos, fetched with scalar loads that depend on blockIdx.z alone) is k_dec_out's
// row - item, ring slot, crop origin, RESULT size, destination offset and strides, colour variant - followed by the two plane
// classes (ScalePlane: source and result size, largest tap counts, the dividers by D, by W and by H) and the tile height.
//
// Form.  A block is one tile of the RESULT: DOS_TW luma columns by th luma rows (th even, chosen by the host so that the tile's
// source rows fit SC_ROWS), and with it the DOS_TW / 2 by th / 2 chroma samples of both chroma planes.  Every layout needs all three:
// the planar ones store them one after the other, NV12 / NV21 weave the two chroma tiles, RGBA converts the luma tile with its
// chroma tile.  Per plane, as k_scale_to_i420_step's scale_tile: 1. the source rows of the tile to LDS as they lie, 16 bytes per
// lane from addresses that are multiples of 16; 2. the horizontal sums of every source row, once; 3. the vertical sums and one
// division per sample, four samples per lane - into an LDS tile of the result instead of memory.  Then 4. the tile goes out by
// k_dec_out's lane map: a lane takes one 16-byte chunk of a DESTINATION row, aligned to 16 bytes there whatever the row's own
// alignment is; a chunk the tile's span of the row covers only in part (the row or the tile starts or ends inside it) is written
// sample by sample, so no byte outside a row is touched and neighbouring tiles never write the same byte.
//
// The source is a window (crop_x, crop_y, w, h) of a ring slot with the store's pitch; chroma rows may start on odd bytes.  A
// 16-byte piece that reaches outside [slot, slot + plane bytes + 256) - every slot is followed by 256 spare bytes (pic_store.h) -
// is read byte by byte inside that range.  The host refuses ratios above 4 : 1; the row and byte counts are clamped to the LDS
// arrays regardless.  No scratch.
#pragma once

// pitches of the result tiles in LDS: a chunk's bytes are read as aligned dwords from the dword below, one dword beyond
enum { DOS_TW = 128, DOS_TH = 32, DOS_YP = DOS_TW + 16, DOS_CP = DOS_TW / 2 + 16 };

struct DecOutScalePos {
    DecOutPos o;       // width, height: the RESULT size
    ScalePlane y, c;   // luma; both chroma planes
    uint32_t th, reserved;
};
static_assert(sizeof(DecOutScalePos) == 200, "DecOutScalePos layout");

namespace dec_out {

// steps 1 to 3 for one plane: result samples [X0, X0 + TW) x [Y0, Y0 + th) of plane P into out (pitch opitch, a multiple of 4).
// src: sample (0, 0) of the window; [lo, hi): what may be read.  Ends with a barrier: s_raw and s_sum are free again.
template <int TW>
__device__ __forceinline__ void scale_tile_lds(const uint8_t* __restrict__ src, int stride, const uint8_t* lo, const uint8_t* hi, const ScalePlane& P, int X0, int Y0, int th,
                                               uint8_t* s_raw, uint32_t* s_sum, uint8_t* out, int opitch)
{
    const int tid = threadIdx.x;
    const int X1 = min(P.w, X0 + TW), Y1 = min(P.h, Y0 + th);
    // source samples [I0, I1), rows [R0, R1)
    const int I0 = (int)scale_divide((uint32_t)(X0 * P.sw), P.dw), I1 = (int)scale_divide((uint32_t)(X1 * P.sw + P.w - 1), P.dw);
    const int R0 = (int)scale_divide((uint32_t)(Y0 * P.sh), P.dh), R1 = min(R0 + SC_ROWS, (int)scale_divide((uint32_t)(Y1 * P.sh + P.h - 1), P.dh));
    const int nrows = R1 - R0, nbytes = min(I1 - I0, SC_PITCH - 16);
    const uint8_t* const row0 = src + (size_t)R0 * stride + I0;
    const uint32_t low0 = (uint32_t)(uintptr_t)row0;

    // 1.  (r, k) = (row, piece of 16 bytes) from a flat index: idx / nch by a multiplication that is exact below 65536 / nch
    const int nch = (nbytes + 30) >> 4, inv = (65536 + nch - 1) / nch;   // nch <= 34, idx < 33 * 34
    for (int idx = tid; idx < nrows * nch; idx += 256) {
        const int r = (idx * inv) >> 16, k = idx - r * nch;
        const uint8_t* const a = row0 + (size_t)r * stride;
        const uint8_t* const p = a - ((uintptr_t)a & 15) + 16 * k;
        if (p >= a + nbytes) continue;
        uint4 v;
        if (p >= lo && p + 16 <= hi) v = *(const uint4*)p;
        else {
            uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (p + b >= lo && p + b < hi) q[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
        *(uint4*)(s_raw + r * SC_PITCH + 16 * k) = v;
    }
    __syncthreads();

    // 2.  column j of the tile, rows 256 / TW at a time
    {
        const int j = tid & (TW - 1), x = X0 + j;
        if (x < X1) {
            int i0, i1, wt[5];
            scale_taps(x, P.sw, P.dw, i0, i1, wt);
            int off[5];
#pragma unroll
            for (int t = 0; t < 5; t++) off[t] = min(min(i0 + t, i1) - I0, nbytes - 1);
            const int ntap = P.tapsx;
            for (int r = tid / TW; r < nrows; r += 256 / TW) {
                const uint8_t* const rr = s_raw + r * SC_PITCH + (int)((low0 + (uint32_t)r * (uint32_t)stride) & 15);
                uint32_t s = (uint32_t)wt[0] * rr[off[0]] + (uint32_t)wt[1] * rr[off[1]];
                if (ntap > 2) s += (uint32_t)wt[2] * rr[off[2]];
                if (ntap > 3) s += (uint32_t)wt[3] * rr[off[3]];
                if (ntap > 4) s += (uint32_t)wt[4] * rr[off[4]];
                s_sum[r * SC_TW + j] = s;
            }
        }
    }
    __syncthreads();

    // 3.  lane = columns 4 q .. 4 q + 3 of a result row (columns at and beyond X1 hold nothing that is ever stored)
    {
        const int q = tid & (TW / 4 - 1), x = X0 + 4 * q;
        const int ntap = P.tapsy;
        const uint32_t half = P.div.d >> 1;
        if (x < X1)
            for (int y = Y0 + tid / (TW / 4); y < Y1; y += 256 / (TW / 4)) {
                int j0, j1, wt[5];
                scale_taps(y, P.sh, P.dh, j0, j1, wt);
                uint32_t n[4] = {0, 0, 0, 0};
                auto tap = [&](int t) {
                    const uint32_t* const rr = s_sum + min(min(j0 + t, j1) - R0, nrows - 1) * SC_TW;
                    const uint4 a = *(const uint4*)(rr + 4 * q);
                    n[0] += (uint32_t)wt[t] * a.x; n[1] += (uint32_t)wt[t] * a.y; n[2] += (uint32_t)wt[t] * a.z; n[3] += (uint32_t)wt[t] * a.w;
                };
                tap(0); tap(1);
                if (ntap > 2) tap(2);
                if (ntap > 3) tap(3);
                if (ntap > 4) tap(4);
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) v |= (scale_divide(n[k] + half, P.div) & 255u) << (8 * k);
                *(uint32_t*)(out + (y - Y0) * opitch + 4 * q) = v;
            }
    }
    __syncthreads();
}

// n (8 or 16) bytes of LDS from s, an address of any alignment: load_bytes on the other address space
template <int N>
__device__ __forceinline__ void lds_bytes(const uint8_t* s, uint32_t* out)
{
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3), sh = 8u * mis;
    const uint32_t* p = (const uint32_t*)(s - mis);
    uint32_t d[N / 4 + 1];
#pragma unroll
    for (int i = 0; i <= N / 4; i++) d[i] = p[i];
#pragma unroll
    for (int i = 0; i < N / 4; i++) out[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> sh);
}

// 4, planes: rows [0, nrows) of an LDS tile whose bytes are bytes [b0, b1) of the destination rows drow0 + r * dstride.  NCH: 16-byte
// chunks a span of b1 - b0 bytes can touch wherever it starts
template <int NCH>
__device__ __forceinline__ void store_plane(const uint8_t* tile, int tpitch, uint8_t* drow0, size_t dstride, int b0, int b1, int nrows)
{
    for (int idx = threadIdx.x; idx < nrows * NCH; idx += 256) {
        const int r = idx / NCH, kc = idx - r * NCH;
        uint8_t* const drow = drow0 + (size_t)r * dstride;
        uint8_t* const a = drow + b0;
        uint8_t* const c = a - ((uintptr_t)a & 15) + 16 * kc;
        const int k = (int)(c - drow);   // the row byte the chunk starts at: b0 - 15 ..
        if (k >= b1) continue;
        const uint8_t* const s = tile + r * tpitch + (k - b0);
        if (k >= b0 && k + 16 <= b1) {
            uint32_t q[4];
            lds_bytes<16>(s, q);
            *(Q4*)c = Q4{q[0], q[1], q[2], q[3]};
            continue;
        }
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (k + i >= b0 && k + i < b1) c[i] = s[i];
    }
}

// 4, NV12 (a = the U tile, b = the V tile) / NV21 (a = V, b = U): bytes [b0, b1) (even) of the rows of a0 b0 a1 b1 ...
template <int NCH>
__device__ __forceinline__ void store_weave(const uint8_t* ta, const uint8_t* tb, int tpitch, uint8_t* drow0, size_t dstride, int b0, int b1, int nrows)
{
    for (int idx = threadIdx.x; idx < nrows * NCH; idx += 256) {
        const int r = idx / NCH, kc = idx - r * NCH;
        uint8_t* const drow = drow0 + (size_t)r * dstride;
        uint8_t* const a = drow + b0;
        uint8_t* const c = a - ((uintptr_t)a & 15) + 16 * kc;
        const int k = (int)(c - drow);   // even
        if (k >= b1) continue;
        const uint8_t* const sa = ta + r * tpitch, * const sb = tb + r * tpitch;
        if (k >= b0 && k + 16 <= b1) {
            uint32_t qa[2], qb[2];
            lds_bytes<8>(sa + (k - b0) / 2, qa);
            lds_bytes<8>(sb + (k - b0) / 2, qb);
            *(Q4*)c = Q4{weave(qa[0], qb[0]), weave(qa[0] >> 16, qb[0] >> 16), weave(qa[1], qb[1]), weave(qa[1] >> 16, qb[1] >> 16)};
            continue;
        }
#pragma unroll
        for (int i = 0; i < 16; i += 2)
            if (k + i >= b0 && k + i < b1) *(uint16_t*)(c + i) = (uint16_t)(sa[(k + i - b0) / 2] | (sb[(k + i - b0) / 2] << 8));
    }
}

// 4, RGBA: pixels [x0, x1) (x0 even) of rows [0, nrows) from the luma tile and the chroma tiles; rows start on 8 bytes, so a chunk
// starts at an even pixel
__device__ __forceinline__ void store_rgba(const OutCoef& K, const uint8_t* ty, const uint8_t* tu, const uint8_t* tv, uint8_t* drow0, size_t dstride, int x0, int x1, int nrows)
{
    constexpr int NCH = DOS_TW / 4 + 1;
    for (int idx = threadIdx.x; idx < nrows * NCH; idx += 256) {
        const int r = idx / NCH, kc = idx - r * NCH;
        uint8_t* const drow = drow0 + (size_t)r * dstride;
        uint8_t* const a = drow + 4 * (size_t)x0;
        uint8_t* const c = a - ((uintptr_t)a & 15) + 16 * kc;
        const int k = (int)(c - drow);   // a multiple of 8
        if (k >= 4 * x1) continue;
        const int x = k / 4 - x0;        // even; pixel of the tile: -2 ..
        const uint8_t* const ys = ty + r * DOS_YP, * const us = tu + (r >> 1) * DOS_CP, * const vs = tv + (r >> 1) * DOS_CP;
        if (x >= 0 && x0 + x + 4 <= x1) {
            const uint32_t y01 = *(const uint16_t*)(ys + x), y23 = *(const uint16_t*)(ys + x + 2);
            const int u0 = us[x / 2], u1 = us[x / 2 + 1], v0 = vs[x / 2], v1 = vs[x / 2 + 1];
            *(Q4*)c = Q4{rgba_pixel(K, (int)(y01 & 255u), u0, v0), rgba_pixel(K, (int)(y01 >> 8), u0, v0), rgba_pixel(K, (int)(y23 & 255u), u1, v1), rgba_pixel(K, (int)(y23 >> 8), u1, v1)};
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (x + i >= 0 && x0 + x + i < x1) *(uint32_t*)(c + 4 * i) = rgba_pixel(K, ys[x + i], us[(x + i) / 2], vs[(x + i) / 2]);
    }
}

}  // namespace dec_out

// grid (tiles across the widest result, tile rows of the position with the most, positions), block 256
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_dec_out_scaled(const DecOutParams P, const DecOutScalePos* __restrict__ tab)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[SC_ROWS * SC_PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_sum[SC_ROWS * SC_TW];
    __shared__ __attribute__((aligned(16))) uint8_t s_y[DOS_TH * DOS_YP];
    __shared__ __attribute__((aligned(16))) uint8_t s_u[(DOS_TH / 2) * DOS_CP];
    __shared__ __attribute__((aligned(16))) uint8_t s_v[(DOS_TH / 2) * DOS_CP];
    const DecOutScalePos t = tab[blockIdx.z];
    const int W = (int)t.o.width, H = (int)t.o.height;
    const int th = min(max((int)t.th & ~1, 2), (int)DOS_TH);
    const int X0 = (int)blockIdx.x * DOS_TW, Y0 = (int)blockIdx.y * th;
    if (X0 >= W || Y0 >= H) return;
    const int X1 = min(W, X0 + DOS_TW), nr = min(H, Y0 + th) - Y0;   // even, both
    const int pitch = P.pitch, cpitch = pitch / 2;
    const size_t ysz = P.st_ring_y - 256, csz = P.st_ring_c - 256;     // bytes of a slot's plane (pic_store.h)
    const uint8_t* const ys = P.y + (size_t)t.o.item * P.st_y + (size_t)t.o.slot * P.st_ring_y;
    const size_t coff = (size_t)t.o.item * P.st_c + (size_t)t.o.slot * P.st_ring_c;
    const size_t cwin = (size_t)(t.o.crop_y / 2) * cpitch + t.o.crop_x / 2;
    dec_out::scale_tile_lds<DOS_TW>(ys + (size_t)t.o.crop_y * pitch + t.o.crop_x, pitch, ys, ys + ysz + 256, t.y, X0, Y0, th, s_raw, s_sum, s_y, DOS_YP);
    dec_out::scale_tile_lds<DOS_TW / 2>(P.u + coff + cwin, cpitch, P.u + coff, P.u + coff + csz + 256, t.c, X0 / 2, Y0 / 2, th / 2, s_raw, s_sum, s_u, DOS_CP);
    dec_out::scale_tile_lds<DOS_TW / 2>(P.v + coff + cwin, cpitch, P.v + coff, P.v + coff + csz + 256, t.c, X0 / 2, Y0 / 2, th / 2, s_raw, s_sum, s_v, DOS_CP);

    uint8_t* const d = P.dst + t.o.off;
    if constexpr (LAYOUT == DEC_OUT_RGBA) {
        dec_out::store_rgba(dec_out::out_coef(t.o.colour), s_y, s_u, s_v, d + (size_t)Y0 * t.o.stride, t.o.stride, X0, X1, nr);
    } else {
        dec_out::store_plane<DOS_TW / 16 + 1>(s_y, DOS_YP, d + (size_t)Y0 * t.o.stride, t.o.stride, X0, X1, nr);
        uint8_t* const dc = d + (size_t)H * t.o.stride + (size_t)(Y0 / 2) * t.o.cstride;
        if constexpr (LAYOUT == DEC_OUT_I420) {
            dec_out::store_plane<DOS_TW / 32 + 1>(s_u, DOS_CP, dc, t.o.cstride, X0 / 2, X1 / 2, nr / 2);
            dec_out::store_plane<DOS_TW / 32 + 1>(s_v, DOS_CP, dc + (size_t)(H / 2) * t.o.cstride, t.o.cstride, X0 / 2, X1 / 2, nr / 2);
        } else {
            dec_out::store_weave<DOS_TW / 16 + 1>(LAYOUT == DEC_OUT_NV12 ? s_u : s_v, LAYOUT == DEC_OUT_NV12 ? s_v : s_u, DOS_CP, dc, t.o.cstride, X0, X1, nr / 2);
        }
    }
}
