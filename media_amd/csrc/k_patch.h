// media_amd/csrc/k_patch.h -- damage tiles (damage.h; include/mi355x_h264.h, "damage tiles"): ONE launch per step writes the tiles
// that the step's damage calls transferred into their streams' staging slots, in front of the scaler, the conversion and the first
// kernel that reads samples.  A step in which no picture has tiles does not launch it.
//
// One wave per tile, lanes move 16 bytes each: a Y tile row is 4 lanes, so 64 lanes cover the 16 rows; chroma takes a second pass
// (I420: lanes 0..15 the 8 U rows, 16..31 the 8 V rows; NV12: lanes 0..31 the 8 interleaved rows).  An RGBA tile row is 16 lanes:
// four passes of four rows.  Tiles at the picture's edge are clipped per row: nothing outside the picture is stored, so nothing
// outside the (tight) slot is.  Loads: the payload's tiles start on 16 bytes and every lane's offset is a multiple of 16.  Stores:
// slots are tight and widths only even, so a destination row may start on any 2-byte boundary (Y, NV12), on any byte (I420 chroma of
// a width with w % 4 == 2) or on 8 bytes (RGBA) - every store tests its own address, as the kernels' source loads do: 16 bytes at
// once only to an address that is a multiple of 16, 4-byte words to one that is a multiple of 4, bytes otherwise.
#pragma once

// a position of the step's patch table (HubCtx::TAB_PATCH): the payload as damage.h packs it, the slot, and the slot's picture
struct PatchSrc { unsigned long long payload, slot; uint32_t ntiles, layout, w, h; };
static_assert(sizeof(PatchSrc) == 32, "the table's stride");

// the first n (1 .. 16) bytes of v to dst
__device__ __forceinline__ void patch_store(uint8_t* dst, const uint4 v, int n)
{
    if (n == 16 && (((uintptr_t)dst) & 15) == 0) { *(uint4*)dst = v; return; }
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    if ((((uintptr_t)dst) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (4 * k + 4 <= n) ((uint32_t*)dst)[k] = wd[k];
            else if (4 * k < n) {
#pragma unroll
                for (int b = 0; b < 4; b++) if (4 * k + b < n) dst[4 * k + b] = (uint8_t)(wd[k] >> (8 * b));
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int b = 0; b < 4; b++) if (4 * k + b < n) dst[4 * k + b] = (uint8_t)(wd[k] >> (8 * b));
}

extern "C" {
// grid: (ceil(most tiles of a position / 4), positions with tiles), 256 threads: wave k of block x takes tile 4 * x + k of position y
__global__ __launch_bounds__(256) void k_patch_step(const PatchSrc* __restrict__ tab)
{
    const PatchSrc T = tab[blockIdx.y];
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= T.ntiles) return;
    const int lane = threadIdx.x & 63;
    const int w = (int)T.w, h = (int)T.h;
    const uint8_t* const pay = (const uint8_t*)(uintptr_t)T.payload;
    uint8_t* const slot = (uint8_t*)(uintptr_t)T.slot;
    const uint32_t t = ((const uint32_t*)(pay + 16))[k];
    const int ntx = (w + 63) >> 6;
    const int x0 = (int)(t % (uint32_t)ntx) * 64, y0 = (int)(t / (uint32_t)ntx) * 16;
    if (x0 >= w || y0 >= h) return;   // (no such tile in this picture: nothing is stored)
    const size_t toff = ((size_t)16 + 4 * (size_t)T.ntiles + 15) & ~(size_t)15;
    if (T.layout == 2) {   // RGBA: 16 rows of 256 bytes
        const uint8_t* const tile = pay + toff + (size_t)k * 4096;
#pragma unroll
        for (int pass = 0; pass < 4; pass++) {
            const int c = pass * 64 + lane, row = c >> 4, px = x0 + (c & 15) * 4;
            if (y0 + row >= h || px >= w) continue;
            const uint4 v = *(const uint4*)(tile + (size_t)c * 16);
            patch_store(slot + ((size_t)(y0 + row) * w + px) * 4, v, min(4, w - px) * 4);
        }
        return;
    }
    const uint8_t* const tile = pay + toff + (size_t)k * 1536;
    {   // Y: 16 rows of 64
        const int row = lane >> 2, x = x0 + (lane & 3) * 16;
        if (y0 + row < h && x < w) {
            const uint4 v = *(const uint4*)(tile + (size_t)lane * 16);
            patch_store(slot + (size_t)(y0 + row) * w + x, v, min(16, w - x));
        }
    }
    const size_t ysz = (size_t)w * h;
    if (T.layout == 1) {   // NV12: 8 interleaved rows of 64
        if (lane >= 32) return;
        const int row = lane >> 2, x = x0 + (lane & 3) * 16;
        if (y0 / 2 + row < h / 2 && x < w) {
            const uint4 v = *(const uint4*)(tile + 1024 + (size_t)lane * 16);
            patch_store(slot + ysz + (size_t)(y0 / 2 + row) * w + x, v, min(16, w - x));
        }
        return;
    }
    if (lane >= 32) return;   // I420: 8 U rows of 32, then 8 V rows of 32
    const int p = lane >> 4, l = lane & 15, row = l >> 1, x = x0 / 2 + (l & 1) * 16, cw = w / 2;
    if (y0 / 2 + row < h / 2 && x < cw) {
        const uint4 v = *(const uint4*)(tile + 1024 + (size_t)lane * 16);
        patch_store(slot + ysz + (size_t)p * (ysz / 4) + (size_t)(y0 / 2 + row) * cw + x, v, min(16, cw - x));
    }
}
}
