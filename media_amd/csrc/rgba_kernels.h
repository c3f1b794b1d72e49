// media_amd/csrc/rgba_kernels.h -- RGBA pictures into the I420 staging picture the encoder kernels read
#pragma once
extern "C" {   // (the kernels' names carry no C++ mangling, as they never did)
// RGBA ingest: one conversion pass into the I420 staging picture (include/mi355x_h264.h states the arithmetic;
// oracle/h264_rgba.c is its CPU restatement).  Thread = one 2x2 block: two 8-byte loads, two 2-byte luma stores, one Cb, one Cr.
__device__ __forceinline__ void rgba_block_to_i420(const uint8_t* __restrict__ rgba, size_t stride, uint8_t* __restrict__ i420, int w, int h, int bx, int by)
{
    uint8_t* const Y = i420;
    uint8_t* const U = i420 + (size_t)w * h;
    uint8_t* const V = U + (size_t)(w / 2) * (h / 2);
    int sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint2 p = *(const uint2*)(rgba + (size_t)(2 * by + r) * stride + 8 * (size_t)bx);   // (rows start on 8 bytes: stride % 8 == 0 checked by the host)
        const int r0 = p.x & 255, g0 = (p.x >> 8) & 255, b0 = (p.x >> 16) & 255;
        const int r1 = p.y & 255, g1 = (p.y >> 8) & 255, b1 = (p.y >> 16) & 255;
        const int y0 = ((66 * r0 + 129 * g0 + 25 * b0 + 128) >> 8) + 16, y1 = ((66 * r1 + 129 * g1 + 25 * b1 + 128) >> 8) + 16;
        *(uint16_t*)(Y + (size_t)(2 * by + r) * w + 2 * bx) = (uint16_t)(y0 | (y1 << 8));
        sr += r0 + r1; sg += g0 + g1; sb += b0 + b1;
    }
    const int r = (sr + 2) >> 2, g = (sg + 2) >> 2, b = (sb + 2) >> 2;
    U[(size_t)by * (w / 2) + bx] = (uint8_t)(((-38 * r - 74 * g + 112 * b + 128) >> 8) + 128);
    V[(size_t)by * (w / 2) + bx] = (uint8_t)(((112 * r - 94 * g - 18 * b + 128) >> 8) + 128);
}
__global__ __launch_bounds__(256) void k_rgba_to_i420(const uint8_t* __restrict__ rgba, size_t stride, uint8_t* __restrict__ i420, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    rgba_block_to_i420(rgba, stride, i420, w, h, bx, by);
}
// The stream hub's form: ONE launch converts every picture of a step.  blockIdx.z = position; tab[position] = where the RGBA picture
// lies (the caller's device memory or the hub's RGBA staging) and its row stride, srctab[position] = the I420 staging slot the
// encoder kernels of the step then read.  Eight bytes per lane and row, as above: rows start on 8 bytes for every even width, so
// widths that are not multiples of 4 take the same path.
struct RgbaSrc { unsigned long long addr, stride; };
__global__ __launch_bounds__(256) void k_rgba_to_i420_step(const RgbaSrc* __restrict__ tab, const unsigned long long* __restrict__ srctab, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    const RgbaSrc t = tab[blockIdx.z];
    rgba_block_to_i420((const uint8_t*)t.addr, (size_t)t.stride, (uint8_t*)srctab[blockIdx.z], w, h, bx, by);
}
}  // extern "C"
