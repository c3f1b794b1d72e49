// media_amd/csrc/k_dec_out.h -- decoder output: the cropped pictures of a call gathered out of the reconstruction ring into ONE
// packed destination, in one launch (include/mi355x_h264_dec.h: mi355x_h264_dec_read, _dec_group_read_all, _dec_group_set_output).
//
// blockIdx.z = position.  tab[position] (DecOutPos, 48 bytes, fetched with scalar loads that depend on blockIdx.z alone) says which
// batch item and ring slot the picture lies in, its crop origin and size, and where it goes: byte offset and row strides inside
// the destination.  The source address is dg_read's: plane base + item * st + slot * st_ring + crop_y * pitch + crop_x.
//
// Layouts (MI355X_H264_PIX_*): 0 I420 = Y, U, V planes; 1 NV12 = Y plane, then rows of U, V pairs; 2 NV21 = Y plane, then rows of
// V, U pairs; 3 RGBA = R, G, B, A bytes with A = 255.  A luma row, an NV12 / NV21 chroma row and an RGBA row have `stride`, an I420
// chroma row has `cstride`; plane heights are tight; bytes between a row's end and the next row's start are never written.
//
// RGBA is this build's own definition (the counterpart of oracle/h264_rgba.c, which states the way in): integer BT.601 studio swing,
//   c = 298 * (Y - 16), d = U - 128, e = V - 128,
//   R = clip255((c + 409 * e + 128) >> 8), G = clip255((c - 100 * d - 208 * e + 128) >> 8), B = clip255((c + 516 * d + 128) >> 8),
// the shift arithmetic; the chroma sample of a 2x2 block serves its four pixels (no interpolation).  That is variant 0 of four
// (include/mi355x_h264.h, "colour description": c = m (Y - o), and rv, gu, gv, bu in place of 409, -100, -208, 516).  A launch may
// carry streams of different descriptions, so the variant is the table row's (DecOutPos.colour): a value every lane of the block
// has from scalar loads, turned into the six coefficients by scalar selects - no table in memory is indexed.
//
// Lane map.  The unit of work is one 16-byte chunk of the DESTINATION, aligned to 16 bytes there: lane x of a wave takes chunk
// 64 * blockIdx.x + x of a row, so a wave's store instruction covers 1 KiB of consecutive destination bytes whatever the row's
// own alignment is.  A wave is one row at a time (threadIdx.y, blockIdx.y and a loop of DEC_OUT_ROWS rows), so which plane a row
// belongs to is wave-uniform.  What a chunk needs from the source differs by layout (the template parameter):
//   planes (I420, the luma of NV12 / NV21): 16 source bytes from an address of any alignment (crops are in units of two samples and
//     I420 chroma rows of width / 2 may start on odd bytes): five dwords from the dword below it, funnel-shifted;
//   NV12 / NV21 chroma: 8 U and 8 V bytes the same way (three dwords each), interleaved in registers;
//   RGBA: 4 pixels = 4 luma bytes (two 2-byte loads: luma rows start on 2 bytes) and 2 + 2 chroma bytes.
// A chunk that a row covers only in part (the row starts or ends inside it: widths that are no multiple of 16, tight rows) is
// written sample by sample (byte, pair, pixel) by the same code path, so every even width is served by one kernel and no byte
// outside a row is touched.  Reads stay inside the planes' allocation: a few bytes beyond the 16 asked for, and every ring slot
// is followed by 256 spare bytes (pic_store.h, st_ring_y / st_ring_c).  No LDS, no scratch.
#pragma once

enum { DEC_OUT_I420 = 0, DEC_OUT_NV12 = 1, DEC_OUT_NV21 = 2, DEC_OUT_RGBA = 3, DEC_OUT_ROWS = 8 };

struct DecOutPos {
    uint32_t item, slot, crop_x, crop_y, width, height, stride, cstride;
    unsigned long long off;   // of the picture's first byte inside the destination (a multiple of 256)
    uint32_t colour;          // RGBA: the variant of the conversion, 0 BT.601 limited, 1 BT.709 limited, 2 BT.601 full, 3 BT.709 full
    uint32_t reserved;
};
static_assert(sizeof(DecOutPos) == 48, "DecOutPos layout");
struct DecOutParams {
    const uint8_t* y; const uint8_t* u; const uint8_t* v;   // the store's plane bases (d_plane_base)
    size_t st_y, st_c, st_ring_y, st_ring_c;               // bytes between items / between the ring slots of an item
    int pitch;                                              // coded width
    uint8_t* dst;
    const DecOutPos* tab;
};

namespace dec_out {

struct alignas(16) Q4 { uint32_t x, y, z, w; };

// n (8 or 16) bytes from s, an address of any alignment, as dwords: aligned dword loads from the dword at or below s
template <int N>
__device__ __forceinline__ void load_bytes(const uint8_t* s, uint32_t* out)
{
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3), sh = 8u * mis;
    const uint32_t* p = (const uint32_t*)(s - mis);   // (pointer arithmetic, not an integer made a pointer: the loads stay global loads)
    uint32_t d[N / 4 + 1];
#pragma unroll
    for (int i = 0; i <= N / 4; i++) d[i] = p[i];
#pragma unroll
    for (int i = 0; i < N / 4; i++) out[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> sh);
}

// clip255(v >> 8), written as clamp to 0 .. 65535, then shift: the same value for every int.  In the other order hipcc packs two
// channels with v_ashr_pk_u8_i32 and takes the upper half of its result for zero, which it was not on the MI355X: the blue byte
// that is OR-ed in there came out wrong for some samples.
__device__ __forceinline__ uint32_t clip255_shr8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 65535 ? 65535 : v)) >> 8; }
// the coefficients of variant v (bit 0: BT.709, bit 1: full range); v is uniform over the block
struct OutCoef { int m, o, rv, gu, gv, bu; };
__device__ __forceinline__ OutCoef out_coef(uint32_t v)
{
    const bool b709 = (v & 1u) != 0, full = (v & 2u) != 0;
    OutCoef k;
    k.m = full ? 256 : 298; k.o = full ? 0 : 16;
    k.rv = full ? (b709 ? 403 : 359) : (b709 ? 459 : 409);
    k.gu = full ? (b709 ? -48 : -88) : (b709 ? -55 : -100);
    k.gv = full ? (b709 ? -120 : -183) : (b709 ? -136 : -208);
    k.bu = full ? (b709 ? 475 : 454) : (b709 ? 541 : 516);
    return k;
}
__device__ __forceinline__ uint32_t rgba_pixel(const OutCoef& k, int y, int u, int v)
{
    const int c = k.m * (y - k.o), d = u - 128, e = v - 128;
    return clip255_shr8(c + k.rv * e + 128) | (clip255_shr8(c + k.gu * d + k.gv * e + 128) << 8) | (clip255_shr8(c + k.bu * d + 128) << 16) | 0xFF000000u;
}
// bytes 0, 1 of a and of b as a0 b0 a1 b1
__device__ __forceinline__ uint32_t weave(uint32_t a, uint32_t b) { return (a & 0xFFu) | ((b & 0xFFu) << 8) | ((a & 0xFF00u) << 8) | ((b & 0xFF00u) << 16); }

// a row of n bytes copied from src to drow (its address in the destination); chunk = the lane's 16-byte chunk of the row
__device__ __forceinline__ void copy_chunk(const uint8_t* src, uint8_t* drow, int n, int chunk)
{
    uint8_t* const c = drow - ((uintptr_t)drow & 15) + 16 * (size_t)chunk;
    const int k = (int)(c - drow);   // the row byte the chunk starts at: -15 .. n
    if (k >= n) return;
    if (k >= 0 && k + 16 <= n) {
        uint32_t q[4];
        load_bytes<16>(src + k, q);
        *(Q4*)c = Q4{q[0], q[1], q[2], q[3]};
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i++)
        if (k + i >= 0 && k + i < n) c[i] = src[k + i];
}

// a chroma row of NV12 (a = U, b = V) / NV21 (a = V, b = U): n = width bytes a0 b0 a1 b1 ...; rows start on even bytes
__device__ __forceinline__ void weave_chunk(const uint8_t* a, const uint8_t* b, uint8_t* drow, int n, int chunk)
{
    uint8_t* const c = drow - ((uintptr_t)drow & 15) + 16 * (size_t)chunk;
    const int k = (int)(c - drow);   // even
    if (k >= n) return;
    if (k >= 0 && k + 16 <= n) {
        uint32_t qa[2], qb[2];
        load_bytes<8>(a + k / 2, qa);
        load_bytes<8>(b + k / 2, qb);
        *(Q4*)c = Q4{weave(qa[0], qb[0]), weave(qa[0] >> 16, qb[0] >> 16), weave(qa[1], qb[1]), weave(qa[1] >> 16, qb[1] >> 16)};
        return;
    }
#pragma unroll
    for (int i = 0; i < 16; i += 2)
        if (k + i >= 0 && k + i < n) *(uint16_t*)(c + i) = (uint16_t)(a[(k + i) / 2] | (b[(k + i) / 2] << 8));
}

// a row of w RGBA pixels from its luma row and the chroma rows of its pair of rows; rows start on 8 bytes, so a chunk starts at an
// even pixel: pixels 0, 1 of it share a chroma sample and so do pixels 2, 3
__device__ __forceinline__ void rgba_chunk(const OutCoef& K, const uint8_t* ys, const uint8_t* us, const uint8_t* vs, uint8_t* drow, int w, int chunk)
{
    uint8_t* const c = drow - ((uintptr_t)drow & 15) + 16 * (size_t)chunk;
    const int k = (int)(c - drow);   // a multiple of 8
    if (k >= 4 * w) return;
    const int x = k / 4;             // even; -2 .. w - 2
    if (x >= 0 && x + 4 <= w) {
        const uint32_t y01 = *(const uint16_t*)(ys + x), y23 = *(const uint16_t*)(ys + x + 2);
        const int u0 = us[x / 2], u1 = us[x / 2 + 1], v0 = vs[x / 2], v1 = vs[x / 2 + 1];
        *(Q4*)c = Q4{rgba_pixel(K, (int)(y01 & 255u), u0, v0), rgba_pixel(K, (int)(y01 >> 8), u0, v0), rgba_pixel(K, (int)(y23 & 255u), u1, v1), rgba_pixel(K, (int)(y23 >> 8), u1, v1)};
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (x + i >= 0 && x + i < w) *(uint32_t*)(c + 4 * i) = rgba_pixel(K, ys[x + i], us[(x + i) / 2], vs[(x + i) / 2]);
}

// row R (0 .. rows(layout) - 1, the planes' rows one after the other) of the picture of table row t: the lane's chunk of it
template <int LAYOUT>
__device__ __forceinline__ void row_chunk(const DecOutParams& P, const DecOutPos& t, int R, int chunk)
{
    const int w = (int)t.width, h = (int)t.height, pitch = P.pitch;
    const uint8_t* const ys = P.y + (size_t)t.item * P.st_y + (size_t)t.slot * P.st_ring_y + (size_t)t.crop_y * pitch + t.crop_x;
    const size_t coff = (size_t)t.item * P.st_c + (size_t)t.slot * P.st_ring_c + (size_t)(t.crop_y / 2) * (pitch / 2) + t.crop_x / 2;
    uint8_t* const d = P.dst + t.off;
    if constexpr (LAYOUT == DEC_OUT_RGBA) {
        if (R >= h) return;
        rgba_chunk(out_coef(t.colour), ys + (size_t)R * pitch, P.u + coff + (size_t)(R / 2) * (pitch / 2), P.v + coff + (size_t)(R / 2) * (pitch / 2), d + (size_t)R * t.stride, w, chunk);
    } else {
        if (R < h) { copy_chunk(ys + (size_t)R * pitch, d + (size_t)R * t.stride, w, chunk); return; }
        const int r = R - h;   // chroma row
        uint8_t* const dc = d + (size_t)h * t.stride;
        if constexpr (LAYOUT == DEC_OUT_I420) {
            if (r >= 2 * (h / 2)) return;
            const bool second = r >= h / 2;
            const int rr = second ? r - h / 2 : r;
            copy_chunk((second ? P.v : P.u) + coff + (size_t)rr * (pitch / 2), dc + (size_t)r * t.cstride, w / 2, chunk);
        } else {
            if (r >= h / 2) return;
            const uint8_t* const us = P.u + coff + (size_t)r * (pitch / 2);
            const uint8_t* const vs = P.v + coff + (size_t)r * (pitch / 2);
            weave_chunk(LAYOUT == DEC_OUT_NV12 ? us : vs, LAYOUT == DEC_OUT_NV12 ? vs : us, dc + (size_t)r * t.cstride, w, chunk);
        }
    }
}

}  // namespace dec_out

// grid (chunks of the widest row / 64, rows of the tallest picture / (4 * DEC_OUT_ROWS), positions), block (64, 4)
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_dec_out(const DecOutParams P)
{
    const DecOutPos t = P.tab[blockIdx.z];
    const int chunk = (int)(blockIdx.x * 64 + threadIdx.x);
    const int R0 = (int)(blockIdx.y * 4 + threadIdx.y) * DEC_OUT_ROWS;
    for (int i = 0; i < DEC_OUT_ROWS; i++) dec_out::row_chunk<LAYOUT>(P, t, R0 + i, chunk);
}
