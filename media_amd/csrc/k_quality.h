// media_amd/csrc/k_quality.h -- the quality report (include/mi355x_h264.h, "quality report"): the sum of squared differences
// between the picture the encoder kernels read and the reconstruction that becomes the next reference, per plane and per
// macroblock, over the display samples alone.  Integer arithmetic only: the result is exact whatever the order of summation.
//
// SSE_SEGS waves per macroblock row of the band, a quarter of the row each (grid.x), one picture per grid.y (IND = false: the batch
// item; IND = true: the position of a hub step, through batch_view<true> - its own ring slot, its own source address).  A wave walks
// its part of the row (with a whole row per wave a lone 1080p picture waited on 120 dependent steps of memory latency); a
// macroblock is one luma word (four samples) per lane and one chroma word per lane of the lower half, laid out as load_src_mb lays
// them out, and the source is read with the same tests (a word where the address allows it, clamped single bytes else), so NV12
// and I420 pictures are read in place from any byte.  The samples the coded size adds (replicated columns and rows) are masked
// out, not skipped: the loads stay uniform.
// Nothing is zeroed on the device and nothing is added up across waves: a wave stores its macroblocks' sums (map, 64 entries to a
// store: a store to pinned memory per macroblock would have every iteration wait for the host link) and its three plane sums
// (part, one triple per wave) with plain stores, straight into the step's pinned memory (as k_pack stores the access unit); the
// host adds the waves of the band's rows up when it finishes the picture.
#pragma once

namespace h264 {

// squared differences of the first n (<= 0: none, >= 4: all) of the four samples packed in a and b, as sum a^2 + sum b^2 - 2 sum ab
// over the bytes that count: three v_dot4_u32_u8 (exact: 32 bits hold 8 * 255^2 many times over)
__device__ __forceinline__ uint32_t sse4(uint32_t a, uint32_t b, int n)
{
    const uint32_t m = n >= 4 ? 0xFFFFFFFFu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
    a &= m; b &= m;
    return __builtin_amdgcn_udot4(a, a, __builtin_amdgcn_udot4(b, b, 0u, false), false) - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}

// four source luma samples, columns gx..gx+3 of row gy: the luma path of load_src_mb (clamped like src_px)
__device__ __forceinline__ uint32_t src_luma4(const FrameParams& P, int gx, int gy)
{
    const int yy = gy < P.h ? gy : P.h - 1;
    const uint8_t* p = P.src + (size_t)yy * P.w + gx;
    if (gx + 3 < P.w && (((uintptr_t)p) & 3) == 0) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) v |= (uint32_t)src_px(P.src, P.w, P.h, gx + k, gy) << (8 * k);
    return v;
}

enum { SSE_SEGS = 4 };   // waves per macroblock row

// part: [item][mbh][SSE_SEGS][3] plane sums (Y, U, V) of a wave's part of a macroblock row; map: [item][mbh * mbw] the macroblock's sum over the three planes
template <bool IND>
__global__ __launch_bounds__(64) void k_sse(FrameParams P0, unsigned long long* __restrict__ part, uint32_t* __restrict__ map)
{
    const int lane = threadIdx.x, pos = blockIdx.y;
    const FrameParams P = batch_view<IND>(P0, pos);
    const int g = batch_item<IND>(P0.itemtab, pos);
    const int seg = (int)blockIdx.x % SSE_SEGS;
    const int my = P.band.row0 + (int)blockIdx.x / SSE_SEGS;   // rows of this instance's band only: a halo import rewrites the rows next to it
    if (my >= P.mbh) return;
    const int per = (P.mbw + SSE_SEGS - 1) / SSE_SEGS, mx0 = seg * per, mx1 = min(P.mbw, mx0 + per);   // (a narrow picture leaves the last waves nothing: they store zeros)
    const int lrow = lane >> 2, lxs = (lane & 3) * 4;                        // luma: 16 rows of four words
    const int pl = (lane >> 4) & 1, crow = (lane >> 1) & 7, cxs = (lane & 1) * 4;   // chroma (lanes 0..31): Cb 8 rows of two words, then Cr
    const int gy = 16 * my + lrow, cgy = 8 * my + crow;
    const int pw = P.w / 2, ph = P.h / 2, cpitch = P.cw / 2;
    const uint8_t* const ry = P.rec[0] + (size_t)gy * P.cw;
    const uint8_t* const rc = rec_chroma(P, pl) + (size_t)cgy * cpitch;      // (never P.rec[lane-dependent])
    uint32_t* const mrow = map + (size_t)g * P.st_mb + (size_t)my * P.mbw;
    const int yn = gy < P.h ? P.w : 0, cn = cgy < ph ? pw : 0;              // display samples of this lane's rows, counted from column 0
    // the four words of a macroblock (chroma: lanes 0..31)
    auto load = [&](int mx, uint32_t& sy, uint32_t& ry4, uint32_t& sc, uint32_t& rc4) {
        const int gx = 16 * mx + lxs, cgx = 8 * mx + cxs;
        sy = src_luma4(P, gx, gy);
        ry4 = *(const uint32_t*)(ry + gx);
        sc = rc4 = 0;
        if (lane < 32) { sc = src_chroma4(P, pl, cgx, cgy); rc4 = *(const uint32_t*)(rc + cgx); }
    };
    // Per lane: the plane sums of its own words (a wave has at most 64 macroblocks: 64 * 4 * 255^2 fits 32 bits, and so does the
    // wave's total); per macroblock ONE reduction, of luma and chroma together, for the map.
    uint32_t ay = 0, ac = 0;
    uint32_t mine = 0;   // lane l keeps the map entry of the wave's macroblock 64 k + l: a row's entries leave in stores of up to 64 words
    uint32_t sy = 0, ry4 = 0, sc = 0, rc4 = 0;
    if (mx0 < mx1) load(mx0, sy, ry4, sc, rc4);
    for (int mx = mx0; mx < mx1; mx++) {
        // the next macroblock's words are asked for before this one's are summed (the last iteration reads its own again)
        uint32_t nsy, nry, nsc, nrc;
        load(mx + 1 < mx1 ? mx + 1 : mx, nsy, nry, nsc, nrc);
        const uint32_t ey = sse4(sy, ry4, yn - (16 * mx + lxs));
        const uint32_t ec = sse4(sc, rc4, cn - (8 * mx + cxs));             // (lanes 32..63 hold zeros)
        ay += ey; ac += ec;
        const uint32_t tot = (uint32_t)wave_sum_dpp((int)(ey + ec));        // at most 384 * 255^2
        const int k = mx - mx0;
        if (lane == (k & 63)) mine = tot;
        if ((k & 63) == 63 || mx == mx1 - 1) {
            if (lane <= (k & 63)) mrow[mx0 + (k & ~63) + lane] = mine;
        }
        sy = nsy; ry4 = nry; sc = nsc; rc4 = nrc;
    }
    const uint32_t ty = (uint32_t)wave_sum_dpp((int)ay);
    const int c16 = row_sum16_dpp((int)ac);
    const uint32_t tu = (uint32_t)__builtin_amdgcn_readlane(c16, 0), tv = (uint32_t)__builtin_amdgcn_readlane(c16, 16);
    if (lane == 0) {   // (64 bits in memory: the host adds a picture's partials up, and a picture's sum does not fit 32)
        unsigned long long* o = part + (((size_t)g * P.mbh + my) * SSE_SEGS + seg) * 3;
        o[0] = ty; o[1] = tu; o[2] = tv;
    }
}

}  // namespace h264
