// media_amd/csrc/scale_kernels.h -- source pictures larger than the coded size, area-resampled into the staging picture the encoder
// kernels read (include/mi355x_h264.h, "scaled streams", states the arithmetic; tests/scale.py is its numpy restatement)
#pragma once

// ---- host: a divider the kernel applies with one multiplication.  n / d for EVERY 32-bit n (Granlund & Montgomery, "Division by
// invariant integers using multiplication", figure 4.1): l = ceil(log2 d), m = floor(2^32 * (2^l - d) / d) + 1, t = mulhi(m, n),
// q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0) ----
struct ScaleDiv { uint32_t d, m, s1, s2; };
inline ScaleDiv scale_div_make(uint32_t d)
{
    uint32_t l = 0;
    while (((uint64_t)1 << l) < d) l++;
    ScaleDiv v;
    v.d = d;
    v.m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - d)) / d + 1);
    v.s1 = l < 1 ? l : 1;
    v.s2 = l > 1 ? l - 1 : 0;
    return v;
}
// one resampled plane of a launch: source and result size in samples, the dividers by D = sw * sh (the result), by w and by h
// (tap positions), and the largest number of taps of a result sample per dimension (2 at 1 : 1 .. 5 above 3 : 1)
struct ScalePlane { int sw, sh, w, h, tapsx, tapsy; ScaleDiv div, dw, dh; };
inline int scale_max_taps(int s, int d) { return std::min(5, (s + d - 1) / d + 1); }
inline ScalePlane scale_plane_make(int sw, int sh, int w, int h)
{
    return ScalePlane{sw, sh, w, h, scale_max_taps(sw, w), scale_max_taps(sh, h), scale_div_make((uint32_t)sw * (uint32_t)sh), scale_div_make((uint32_t)w), scale_div_make((uint32_t)h)};
}

// where a position's source picture lies (tight, in the layout named) and its row strides in bytes: first plane, chroma plane(s)
struct ScaleSrc { unsigned long long addr; uint32_t stride, stride_c, layout, pad; };

// the tile of one workgroup: SC_TW bytes of a result row as the source interleaves them (planar: 128 samples; NV12 chroma: 64 Cb Cr
// pairs; RGBA: 32 pixels) by th rows.  At the 4 : 1 limit that is at most 516 source bytes, and always at most 33 rows (SC_PITCH: plus
// up to 15 bytes in front, the row's distance from a multiple of 16).
enum { SC_TW = 128, SC_ROWS = 33, SC_CHUNKS = 34, SC_PITCH = 16 * SC_CHUNKS };
// result rows per tile: as many as SC_ROWS source rows serve (th * sh / h + 2 <= 33: 8 at 4 : 1, 20 at 3 : 2), at most 32
inline int scale_tile_rows(int sh, int h) { return std::min(32, std::max(8, (SC_ROWS - 2) * h / sh)); }
inline int scale_tiles_x(int w, int comps) { return (w * comps + SC_TW - 1) / SC_TW; }

__device__ __forceinline__ uint32_t scale_divide(uint32_t n, const ScaleDiv& v)
{
    const uint32_t t = __umulhi(v.m, n);
    return (t + ((n - t) >> v.s1)) >> v.s2;
}

// the taps of result sample x on an axis of `s` source samples resampled to dv.d: first source sample, last one, and the integer
// overlap lengths wt[0 .. 4] (0 past the last; they sum to s)
__device__ __forceinline__ void scale_taps(int x, int s, const ScaleDiv& dv, int& i0, int& i1, int wt[5])
{
    const int d = (int)dv.d, lo = x * s, hi = lo + s;
    i0 = (int)scale_divide((uint32_t)lo, dv); i1 = (int)scale_divide((uint32_t)(hi + d - 1), dv) - 1;
#pragma unroll
    for (int t = 0; t < 5; t++) {
        const int a = (i0 + t) * d;
        wt[t] = i0 + t <= i1 ? min(hi, a + d) - max(lo, a) : 0;
    }
}

// One tile of one plane.  LOG2C: log2 of the components a source sample interleaves (0 planar, 1 NV12 chroma, 2 RGBA).
//   1. the source rows of the tile go to LDS as they lie, 16 bytes per lane from addresses that are multiples of 16; a piece that
//      reaches outside [pic, pic_end) - the picture's first or last bytes, when it does not start on 16 - goes byte by byte
//   2. the horizontal sums of every source row, once (column j = result sample j >> LOG2C, component j & (C - 1))
//   3. every result row from the (at most 5) rows of sums it covers, divided once, stored as words
// Taps beyond the plane's largest count (P.tapsx, P.tapsy: the same for every lane) have weight 0 everywhere and are skipped.
// dst0 / dst1: planar and RGBA: dst0 is the result plane (pitch dpitch bytes); NV12: dst0 the Cb plane, dst1 the Cr plane.
template <int LOG2C>
__device__ __forceinline__ void scale_tile(const uint8_t* __restrict__ src, uint32_t stride, const uint8_t* pic, const uint8_t* pic_end, const ScalePlane& P,
                                           uint8_t* __restrict__ dst0, uint8_t* __restrict__ dst1, int dpitch, int tx, int ty, int th, uint8_t* s_raw, uint32_t* s_sum)
{
    constexpr int C = 1 << LOG2C;
    const int tid = threadIdx.x;
    const int X0 = tx * (SC_TW >> LOG2C), Y0 = ty * th;                 // first result sample and row of the tile
    const int X1 = min(P.w, X0 + (SC_TW >> LOG2C)), Y1 = min(P.h, Y0 + th);
    // source samples [I0, I1), rows [R0, R1)
    const int I0 = (int)scale_divide((uint32_t)(X0 * P.sw), P.dw), I1 = (int)scale_divide((uint32_t)(X1 * P.sw + P.w - 1), P.dw);
    const int R0 = (int)scale_divide((uint32_t)(Y0 * P.sh), P.dh), R1 = min(R0 + SC_ROWS, (int)scale_divide((uint32_t)(Y1 * P.sh + P.h - 1), P.dh));
    const int nrows = R1 - R0, nbytes = min((I1 - I0) << LOG2C, SC_PITCH - 16);
    const uint8_t* const row0 = src + (size_t)R0 * stride + ((size_t)I0 << LOG2C);
    const uint32_t low0 = (uint32_t)(uintptr_t)row0;   // (a row's distance from a multiple of 16 needs the low address bits only)

    // 1.  (r, k) = (row, piece of 16 bytes) from a flat index: idx / nch by a multiplication that is exact below 65536 / nch
    const int nch = (nbytes + 30) >> 4, inv = (65536 + nch - 1) / nch;   // nch <= 34, idx < 33 * 34
    for (int idx = tid; idx < nrows * nch; idx += blockDim.x) {
        const int r = (idx * inv) >> 16, k = idx - r * nch;
        const uint8_t* const a = row0 + (size_t)r * stride;
        const uint8_t* const p = a - ((uintptr_t)a & 15) + 16 * k;
        if (p >= a + nbytes) continue;
        uint4 v;
        if (p >= pic && p + 16 <= pic_end) v = *(const uint4*)p;
        else {
            uint32_t q[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; b++)
                if (p + b >= pic && p + b < pic_end) q[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
            v = make_uint4(q[0], q[1], q[2], q[3]);
        }
        *(uint4*)(s_raw + r * SC_PITCH + 16 * k) = v;
    }
    __syncthreads();

    // 2.
    {
        const int j = tid & (SC_TW - 1), x = X0 + (j >> LOG2C), c = j & (C - 1);
        if (x < X1) {
            int i0, i1, wt[5];
            scale_taps(x, P.sw, P.dw, i0, i1, wt);
            int off[5];
#pragma unroll
            for (int t = 0; t < 5; t++) off[t] = ((min(i0 + t, i1) - I0) << LOG2C) + c;
            const int ntap = P.tapsx;
            for (int r = tid / SC_TW; r < nrows; r += blockDim.x / SC_TW) {
                const uint8_t* const rr = s_raw + r * SC_PITCH + (int)((low0 + (uint32_t)r * stride) & 15);
                uint32_t s = (uint32_t)wt[0] * rr[off[0]] + (uint32_t)wt[1] * rr[off[1]];
                if (ntap > 2) s += (uint32_t)wt[2] * rr[off[2]];
                if (ntap > 3) s += (uint32_t)wt[3] * rr[off[3]];
                if (ntap > 4) s += (uint32_t)wt[4] * rr[off[4]];
                s_sum[r * SC_TW + j] = s;
            }
        }
    }
    __syncthreads();

    // 3.  lane = one word of a result row: planar and RGBA columns 4 q .. 4 q + 3; NV12 component q & 1 of four pairs
    {
        const int q = tid & (SC_TW / 4 - 1);
        const int x = X0 + (LOG2C == 0 ? 4 * q : LOG2C == 1 ? 4 * (q >> 1) : q);   // first result sample of the word (RGBA: the pixel)
        const int ntap = P.tapsy;
        const uint32_t half = P.div.d >> 1;
        if (x < X1)
            for (int y = Y0 + tid / (SC_TW / 4); y < Y1; y += blockDim.x / (SC_TW / 4)) {
                int j0, j1, wt[5];
                scale_taps(y, P.sh, P.dh, j0, j1, wt);
                uint32_t n[4] = {0, 0, 0, 0};
                auto tap = [&](int t) {
                    const uint32_t* const rr = s_sum + (min(j0 + t, j1) - R0) * SC_TW;
                    if (LOG2C == 1) {   // eight columns: four Cb Cr pairs, this lane's component
                        const uint4 a = *(const uint4*)(rr + 8 * (q >> 1)), b = *(const uint4*)(rr + 8 * (q >> 1) + 4);
                        const bool cr = q & 1;
                        n[0] += (uint32_t)wt[t] * (cr ? a.y : a.x); n[1] += (uint32_t)wt[t] * (cr ? a.w : a.z);
                        n[2] += (uint32_t)wt[t] * (cr ? b.y : b.x); n[3] += (uint32_t)wt[t] * (cr ? b.w : b.z);
                    } else {
                        const uint4 a = *(const uint4*)(rr + 4 * q);
                        n[0] += (uint32_t)wt[t] * a.x; n[1] += (uint32_t)wt[t] * a.y; n[2] += (uint32_t)wt[t] * a.z; n[3] += (uint32_t)wt[t] * a.w;
                    }
                };
                tap(0); tap(1);
                if (ntap > 2) tap(2);
                if (ntap > 3) tap(3);
                if (ntap > 4) tap(4);
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) v |= scale_divide(n[k] + half, P.div) << (8 * k);
                if (LOG2C == 2) *(uint32_t*)(dst0 + (size_t)y * dpitch + 4 * (size_t)x) = v;   // (a pixel; the alpha byte is resampled too and never read)
                else {
                    uint8_t* const o = ((LOG2C == 1 && (q & 1)) ? dst1 : dst0) + (size_t)y * dpitch + x;
                    if (x + 3 < X1 && ((uintptr_t)o & 3) == 0) *(uint32_t*)o = v;
                    else
                        for (int k = 0; k < 4 && x + k < X1; k++) o[k] = (uint8_t)(v >> (8 * k));
                }
            }
    }
}

extern "C" {
// The stream hub's scaling ingest: ONE launch resamples every picture of a step, all planes.  blockIdx.z = position, tab[position] =
// the source picture, dsttab[position * dst_step] = where the result goes: the tight I420 staging picture of w x h the encoder
// kernels then read (I420, NV12), or the tight RGBA staging picture of w x h that k_rgba_to_i420_step then converts (RGBA).
// blockIdx.x counts tile columns: ntx_y of the first plane (Y, or the RGBA picture), then ntx_c of each chroma plane (NV12: of the
// one interleaved plane); blockIdx.y is the tile row, and a chroma tile below its plane's last row has nothing to do.
// Y and Cp hold the two plane classes; a block picks one by its tile column, never by a lane's or a position's value.
__global__ __launch_bounds__(256) void k_scale_to_i420_step(const ScaleSrc* __restrict__ tab, const unsigned long long* __restrict__ dsttab, int dst_step,
                                                            ScalePlane Y, ScalePlane Cp, int ntx_y, int ntx_c, int th)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[SC_ROWS * SC_PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_sum[SC_ROWS * SC_TW];
    const int b = blockIdx.x, ty = blockIdx.y;
    if (b >= ntx_y && ty * th >= Cp.h) return;
    const ScaleSrc t = tab[blockIdx.z];
    const int layout = __builtin_amdgcn_readfirstlane((int)t.layout);
    const uint8_t* const pic = (const uint8_t*)t.addr;
    uint8_t* const dst = (uint8_t*)dsttab[(size_t)blockIdx.z * dst_step];
    if (layout == PIC_RGBA) {
        scale_tile<2>(pic, t.stride, pic, pic + (size_t)t.stride * Y.sh, Y, dst, nullptr, 4 * Y.w, b, ty, th, s_raw, s_sum);
        return;
    }
    const size_t ysz = (size_t)t.stride * Y.sh, csz = (size_t)t.stride_c * Cp.sh;
    const uint8_t* const pic_end = pic + ysz + (layout == PIC_NV12 ? csz : 2 * csz);
    uint8_t* const dst_u = dst + (size_t)Y.w * Y.h, * const dst_v = dst_u + (size_t)Cp.w * Cp.h;
    if (b < ntx_y) scale_tile<0>(pic, t.stride, pic, pic_end, Y, dst, nullptr, Y.w, b, ty, th, s_raw, s_sum);
    else if (layout == PIC_NV12) scale_tile<1>(pic + ysz, t.stride_c, pic, pic_end, Cp, dst_u, dst_v, Cp.w, b - ntx_y, ty, th, s_raw, s_sum);
    else {
        const int pl = b - ntx_y >= ntx_c ? 1 : 0;
        scale_tile<0>(pic + ysz + (pl ? csz : 0), t.stride_c, pic, pic_end, Cp, pl ? dst_v : dst_u, nullptr, Cp.w, b - ntx_y - pl * ntx_c, ty, th, s_raw, s_sum);
    }
}
}  // extern "C"
