// media_amd/csrc/rgba_kernels.h -- RGBA pictures into the I420 staging picture the encoder kernels read
#pragma once
// The four variants of the conversion (include/mi355x_h264.h, "colour description"; index = colour_variant() of host_framing.h):
// compile-time constants of an instantiation, so every variant is the undescribed kernel with other immediates.  Variant 0 is the
// arithmetic there has always been, and the only one an undescribed stream runs.
template <int V> struct RgbaCoef;
template <> struct RgbaCoef<0> { static constexpr int ya = 66, yb = 129, yc = 25, yo = 16, ud = -38, ue = -74, uf = 112, vd = 112, ve = -94, vf = -18; static constexpr bool full = false; };
template <> struct RgbaCoef<1> { static constexpr int ya = 47, yb = 157, yc = 16, yo = 16, ud = -26, ue = -86, uf = 112, vd = 112, ve = -102, vf = -10; static constexpr bool full = false; };
template <> struct RgbaCoef<2> { static constexpr int ya = 77, yb = 150, yc = 29, yo = 0, ud = -43, ue = -85, uf = 128, vd = 128, ve = -107, vf = -21; static constexpr bool full = true; };
template <> struct RgbaCoef<3> { static constexpr int ya = 54, yb = 183, yc = 19, yo = 0, ud = -29, ue = -99, uf = 128, vd = 128, ve = -116, vf = -12; static constexpr bool full = true; };
// a chroma sample of a full-range variant reaches 256 (b = 255 with r = g = 0 in Cb, r = 255 with g = b = 0 in Cr): the one value
// any variant computes outside 0..255 (tests/test_colour_oracle.py walks the cube), so this is the whole clip
template <int V> __device__ __forceinline__ int rgba_chroma_clip(int c) { if constexpr (RgbaCoef<V>::full) return c > 255 ? 255 : c; else return c; }

// RGBA ingest: one conversion pass into the I420 staging picture (include/mi355x_h264.h states the arithmetic;
// oracle/h264_rgba.c is its CPU restatement).  Thread = one 2x2 block: two 8-byte loads, two 2-byte luma stores, one Cb, one Cr.
template <int V>
__device__ __forceinline__ void rgba_block_to_i420(const uint8_t* __restrict__ rgba, size_t stride, uint8_t* __restrict__ i420, int w, int h, int bx, int by)
{
    using K = RgbaCoef<V>;
    uint8_t* const Y = i420;
    uint8_t* const U = i420 + (size_t)w * h;
    uint8_t* const V_ = U + (size_t)(w / 2) * (h / 2);
    int sr = 0, sg = 0, sb = 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const uint2 p = *(const uint2*)(rgba + (size_t)(2 * by + r) * stride + 8 * (size_t)bx);   // (rows start on 8 bytes: stride % 8 == 0 checked by the host)
        const int r0 = p.x & 255, g0 = (p.x >> 8) & 255, b0 = (p.x >> 16) & 255;
        const int r1 = p.y & 255, g1 = (p.y >> 8) & 255, b1 = (p.y >> 16) & 255;
        const int y0 = ((K::ya * r0 + K::yb * g0 + K::yc * b0 + 128) >> 8) + K::yo, y1 = ((K::ya * r1 + K::yb * g1 + K::yc * b1 + 128) >> 8) + K::yo;
        *(uint16_t*)(Y + (size_t)(2 * by + r) * w + 2 * bx) = (uint16_t)(y0 | (y1 << 8));
        sr += r0 + r1; sg += g0 + g1; sb += b0 + b1;
    }
    const int r = (sr + 2) >> 2, g = (sg + 2) >> 2, b = (sb + 2) >> 2;
    U[(size_t)by * (w / 2) + bx] = (uint8_t)rgba_chroma_clip<V>(((K::ud * r + K::ue * g + K::uf * b + 128) >> 8) + 128);
    V_[(size_t)by * (w / 2) + bx] = (uint8_t)rgba_chroma_clip<V>(((K::vd * r + K::ve * g + K::vf * b + 128) >> 8) + 128);
}
// The stream hub's form: ONE launch converts every picture of a step.  blockIdx.z = position; tab[position] = where the RGBA picture
// lies (the caller's device memory or the hub's RGBA staging) and its row stride, srctab[position] = the I420 staging slot the
// encoder kernels of the step then read.  Eight bytes per lane and row, as above: rows start on 8 bytes for every even width, so
// widths that are not multiples of 4 take the same path.
struct RgbaSrc { unsigned long long addr, stride; };

extern "C" {   // (the kernels' names carry no C++ mangling, as they never did)
__global__ __launch_bounds__(256) void k_rgba_to_i420(const uint8_t* __restrict__ rgba, size_t stride, uint8_t* __restrict__ i420, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    rgba_block_to_i420<0>(rgba, stride, i420, w, h, bx, by);
}
__global__ __launch_bounds__(256) void k_rgba_to_i420_step(const RgbaSrc* __restrict__ tab, const unsigned long long* __restrict__ srctab, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    const RgbaSrc t = tab[blockIdx.z];
    rgba_block_to_i420<0>((const uint8_t*)t.addr, (size_t)t.stride, (uint8_t*)srctab[blockIdx.z], w, h, bx, by);
}
}  // extern "C"

// the same two kernels for the variants a description selects (V = 1, 2, 3): a stream's description belongs to its engine, so a
// launch has one variant, chosen on the host
template <int V>
__global__ __launch_bounds__(256) void k_rgba_to_i420_colour(const uint8_t* __restrict__ rgba, size_t stride, uint8_t* __restrict__ i420, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    rgba_block_to_i420<V>(rgba, stride, i420, w, h, bx, by);
}
template <int V>
__global__ __launch_bounds__(256) void k_rgba_to_i420_step_colour(const RgbaSrc* __restrict__ tab, const unsigned long long* __restrict__ srctab, int w, int h)
{
    const int bx = blockIdx.x * blockDim.x + threadIdx.x, by = blockIdx.y;
    if (bx >= w / 2) return;
    const RgbaSrc t = tab[blockIdx.z];
    rgba_block_to_i420<V>((const uint8_t*)t.addr, (size_t)t.stride, (uint8_t*)srctab[blockIdx.z], w, h, bx, by);
}

// one picture (grid (blocks of 256 block columns, block rows)) or the pictures of a step (grid.z = positions) with variant v
inline void launch_rgba_to_i420(int v, dim3 grid, hipStream_t st, const uint8_t* rgba, size_t stride, uint8_t* i420, int w, int h)
{
    switch (v) {
        case 1: hipLaunchKernelGGL(k_rgba_to_i420_colour<1>, grid, dim3(256), 0, st, rgba, stride, i420, w, h); break;
        case 2: hipLaunchKernelGGL(k_rgba_to_i420_colour<2>, grid, dim3(256), 0, st, rgba, stride, i420, w, h); break;
        case 3: hipLaunchKernelGGL(k_rgba_to_i420_colour<3>, grid, dim3(256), 0, st, rgba, stride, i420, w, h); break;
        default: hipLaunchKernelGGL(k_rgba_to_i420, grid, dim3(256), 0, st, rgba, stride, i420, w, h); break;
    }
}
inline void launch_rgba_to_i420_step(int v, dim3 grid, hipStream_t st, const RgbaSrc* tab, const unsigned long long* srctab, int w, int h)
{
    switch (v) {
        case 1: hipLaunchKernelGGL(k_rgba_to_i420_step_colour<1>, grid, dim3(256), 0, st, tab, srctab, w, h); break;
        case 2: hipLaunchKernelGGL(k_rgba_to_i420_step_colour<2>, grid, dim3(256), 0, st, tab, srctab, w, h); break;
        case 3: hipLaunchKernelGGL(k_rgba_to_i420_step_colour<3>, grid, dim3(256), 0, st, tab, srctab, w, h); break;
        default: hipLaunchKernelGGL(k_rgba_to_i420_step, grid, dim3(256), 0, st, tab, srctab, w, h); break;
    }
}
