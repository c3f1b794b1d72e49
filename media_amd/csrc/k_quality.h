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

// ---- SSIM (include/mi355x_h264.h, "quality report: SSIM"): Q16 integers per 8x8 window at every (4i, 4j), per plane and, for
// luma, per macroblock.  Exact like the SSE: every term is an integer, so the result does not depend on the order of summation.
//
// Waves over (macroblock row, segment) as in k_sse, SSIM_SEGS of them to a row.  A lane is one 4x4 BLOCK of a macroblock: lanes 0..24 the 5x5 luma blocks at
// (4 bx, 4 by) from the macroblock's origin (column 4 and row 4 are the next macroblock's and the next row's first blocks, loaded
// again rather than handed between waves), lanes 32..40 the 3x3 blocks of Cb, lanes 48..56 those of Cr.  A lane reads its block as four
// source words (src_luma4 / src_chroma4: in place, from any byte) and four reconstruction words and keeps the block's sums s1, s2,
// ss, s12 (v_dot4_u32_u8).  A window is 2x2 blocks: the lane of its upper left block fetches the other three (ds_bpermute; s1 and
// s2 travel in one word) and evaluates it.  A window that does not lie wholly inside the display samples (the band's limit for a
// band instance) is masked out whole, never shortened; the loads behind it are clamped into the picture, so they stay uniform.
// The two divisions: the numerators are below 2^47 in magnitude and the divisors between 416 and 2^30, so both are doubles exactly;
// the quotient is computed in double precision (one correctly rounded division), floored, and then CORRECTED by one step from the
// integer remainder n - q d (exact in 64 bits).  The rounded quotient is within 1 of the true one, so a single step either way gives
// the floor whatever the rounding did; nothing rests on the rounding mode.  (The 64-bit integer division is exact as well and was
// measured slower: DESIGN.md section 8.)
// Results as in k_sse: plain stores into the step's pinned memory, one int64 triple per wave, map entries in stores of up to 64 words.
enum { SSIM_C1 = 416, SSIM_C2 = 235963 };
enum { SSIM_SEGS = 8 };   // waves per macroblock row (measured at 1080p, DESIGN.md section 8: 4, 8 and 16 give 37 / 22 / 16 us for a lone picture and 374 / 296 / 365 us for 32)

// floor(n / d) for |n| < 2^47, 416 <= d < 2^30; the quotient fits 18 bits
__device__ __forceinline__ int ssim_floor_div(long long n, int d)
{
#ifdef SSIM_AB_IDIV   // A/B build (Makefile target `ab`): the 64-bit integer division as the compiler expands it, measured in DESIGN.md section 8
    const long long t = n / (long long)d;
    return (int)(n - t * (long long)d < 0 ? t - 1 : t);
#else
    int q = (int)floor((double)n / (double)d);
    const long long r = n - (long long)q * (long long)d;
    q += r < 0 ? -1 : (r >= (long long)d ? 1 : 0);
    return q;
#endif
}

// the window of four blocks: s = s1 | s2 << 16 (each at most 16 * 255), ss = sum of src^2 + rec^2, s12 = sum of src * rec
__device__ __forceinline__ int ssim_window(uint32_t s, uint32_t ss, uint32_t s12)
{
    const int s1 = (int)(s & 0xFFFFu), s2 = (int)(s >> 16);
    const int vars = 64 * (int)ss - s1 * s1 - s2 * s2;
    const int covar = 64 * (int)s12 - s1 * s2;
    const int l = ssim_floor_div((long long)(2 * s1 * s2 + SSIM_C1) << 16, s1 * s1 + s2 * s2 + SSIM_C1);
    const int c = ssim_floor_div((long long)(2 * covar + SSIM_C2) * 65536, vars + SSIM_C2);
    return (int)(((long long)l * (long long)c) >> 16);
}

// part: [item][mbh][SSIM_SEGS][3] plane sums (Y, U, V) of the windows whose origin lies in a wave's part of a macroblock row;
// map: [item][mbh * mbw] the sum of the luma windows whose origin lies in the macroblock
template <bool IND>
__global__ __launch_bounds__(64) void k_ssim(FrameParams P0, long long* __restrict__ part, int32_t* __restrict__ map)
{
    const int lane = threadIdx.x, pos = blockIdx.y;
    const FrameParams P = batch_view<IND>(P0, pos);
    const int g = batch_item<IND>(P0.itemtab, pos);
    const int seg = (int)blockIdx.x % SSIM_SEGS;
    const int my = P.band.row0 + (int)blockIdx.x / SSIM_SEGS;
    if (my >= P.mbh) return;
    const int per = (P.mbw + SSIM_SEGS - 1) / SSIM_SEGS, mx0 = seg * per, mx1 = min(P.mbw, mx0 + per);
    const bool luma = lane < 32;
    const int pl = (lane >> 4) & 1;                          // chroma lanes: 32..47 Cb, 48..63 Cr
    const int idx = luma ? lane : (lane & 15), nb = luma ? 5 : 3;
    const bool live = idx < nb * nb;                         // (the other lanes load block 0 again and count nothing)
    const int bx = live ? idx % nb : 0, by = live ? idx / nb : 0;
    const int mbs = luma ? 16 : 8;                           // samples of a macroblock per axis
    const int pw = luma ? P.w : P.w / 2, ph = luma ? P.h : P.h / 2, pitch = luma ? P.cw : P.cw / 2, prow = luma ? P.ch : P.ch / 2;
    const int lim = min(ph, mbs * (P.band.row0 + P.band.rows));   // a band instance: its own rows (no window straddles two bands)
    const int y0 = mbs * my + 4 * by;                        // first row of the block
    const bool rowok = live && bx < nb - 1 && by < nb - 1 && y0 + 8 <= lim;
    const uint8_t* const rbase = luma ? P.rec[0] : rec_chroma(P, pl);   // (never P.rec[lane-dependent])
    const int o1 = lane + 1, o2 = lane + nb, o3 = lane + nb + 1;        // the blocks to the right, below and below right
    int32_t* const mrow = map + (size_t)g * P.st_mb + (size_t)my * P.mbw;
    // the eight words of a block: rows y0 .. y0 + 3 at column x of its plane
    auto load = [&](int mx, uint32_t (&a)[4], uint32_t (&b)[4]) {
        const int x = mbs * mx + 4 * bx, xr = min(x, pitch - 4);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = y0 + r;
            a[r] = luma ? src_luma4(P, x, y) : src_chroma4(P, pl, x, y);
            b[r] = *(const uint32_t*)(rbase + (size_t)min(y, prow - 1) * pitch + xr);
        }
    };
    int acc = 0;     // this lane's windows: a wave has at most mbw / 4 + 1 macroblocks of 65536 at most each
    int mine = 0;    // lane l keeps the map entry of the wave's macroblock 64 k + l
    uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (mx0 < mx1) load(mx0, a, b);
    for (int mx = mx0; mx < mx1; mx++) {
        // the next macroblock's words are asked for before this one's are summed (the last iteration reads its own again)
        uint32_t na[4], nb4[4];
        load(mx + 1 < mx1 ? mx + 1 : mx, na, nb4);
        uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            s1 = __builtin_amdgcn_udot4(a[r], 0x01010101u, s1, false);
            s2 = __builtin_amdgcn_udot4(b[r], 0x01010101u, s2, false);
            ss = __builtin_amdgcn_udot4(a[r], a[r], __builtin_amdgcn_udot4(b[r], b[r], ss, false), false);
            s12 = __builtin_amdgcn_udot4(a[r], b[r], s12, false);
        }
        uint32_t s = s1 | (s2 << 16);
        s += (uint32_t)__shfl((int)s, o1) + (uint32_t)__shfl((int)s, o2) + (uint32_t)__shfl((int)s, o3);   // (halves of at most 65280: no carry)
        ss += (uint32_t)__shfl((int)ss, o1) + (uint32_t)__shfl((int)ss, o2) + (uint32_t)__shfl((int)ss, o3);
        s12 += (uint32_t)__shfl((int)s12, o1) + (uint32_t)__shfl((int)s12, o2) + (uint32_t)__shfl((int)s12, o3);
        const bool counts = rowok && mbs * mx + 4 * bx + 8 <= pw;
        const int q = counts ? ssim_window(s, ss, s12) : 0;
        acc += q;
        const int r16 = row_sum16_dpp(luma ? q : 0);
        const int tot = __builtin_amdgcn_readlane(r16, 0) + __builtin_amdgcn_readlane(r16, 16);   // at most 16 * 65536 in magnitude
        const int k = mx - mx0;
        if (lane == (k & 63)) mine = tot;
        if ((k & 63) == 63 || mx == mx1 - 1) {
            if (lane <= (k & 63)) mrow[mx0 + (k & ~63) + lane] = mine;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) { a[r] = na[r]; b[r] = nb4[r]; }
    }
    const int t16 = row_sum16_dpp(acc);
    const long long ty = (long long)__builtin_amdgcn_readlane(t16, 0) + (long long)__builtin_amdgcn_readlane(t16, 16);
    const long long tu = __builtin_amdgcn_readlane(t16, 32), tv = __builtin_amdgcn_readlane(t16, 48);
    if (lane == 0) {
        long long* o = part + (((size_t)g * P.mbh + my) * SSIM_SEGS + seg) * 3;
        o[0] = ty; o[1] = tu; o[2] = tv;
    }
}

}  // namespace h264
