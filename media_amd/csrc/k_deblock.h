// media_amd/csrc/k_deblock.h -- in-loop deblocking filter (H.264 8.7).  Macroblock (mx,my)
// filters against samples already finished by its left, top and top-right neighbours, which
// 8.7 orders strictly (vertical edges of a macroblock, then its horizontal edges, macroblocks
// in raster order).  Three forms, same results:
//   k_deblock_pairs one launch, one persistent wave per TWO macroblock rows: the default from a lockstep batch of 8 pictures on
//   k_deblock_rows  one launch, one persistent wave per macroblock row: smaller batches, pictures of several slices, the
//                   latency mode, the decoder peer.  Both are built from one set of per-macroblock steps (db_* further down).
//   k_deblock_pairs_p, k_deblock_rows_p  the encoder's P steps: the same two, each picture with or without the bS 4 filter
//   k_deblock_diag  (first form; MI355X_H264_DIAG=1) one wavefront per macroblock, one launch
//                   per wavefront step mx + 2*my == s
//
// SURVEY.md 8a row a6.4 (iLoopFilterDisableIdc = 0 at
// /root/reference/video_codec/VideoEncoderOpenH264.cpp:295; alpha/beta offsets 0).
//
// Each step's macroblocks touch disjoint samples: own 16x16 (+8x8 chroma), the
// left neighbour's last 3 luma / 1 chroma columns, the top neighbour's last 3
// luma / 1 chroma rows.
#pragma once
#include "dev_common.h"

namespace h264 {

__constant__ const uint8_t c_alpha[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,   0,   0,   0,   4,   4,
                                          5,  6,  7,  8,  9,  10, 12, 13, 15, 17, 20, 22, 25,  28,  32,  36,  40,  45,
                                          50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
__constant__ const uint8_t c_beta[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  2,  2,
                                         2,  3,  3,  3,  3,  4,  4,  4,  6,  6,  7,  7,  8,  8,  9,  9,  10, 10,
                                         11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
__constant__ const uint8_t c_tc0[52][3] = {
    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},    {0, 0, 0},    {0, 0, 0},    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},  {0, 0, 0},
    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},    {0, 0, 0},    {0, 0, 0},    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},  {0, 0, 1},
    {0, 0, 1},   {0, 0, 1},   {0, 0, 1},    {0, 1, 1},    {0, 1, 1},    {1, 1, 1},   {1, 1, 1},   {1, 1, 1},  {1, 1, 1},
    {1, 1, 2},   {1, 1, 2},   {1, 1, 2},    {1, 1, 2},    {1, 2, 3},    {1, 2, 3},   {2, 2, 3},   {2, 2, 4},  {2, 3, 4},
    {2, 3, 4},   {3, 3, 5},   {3, 4, 6},    {3, 4, 6},    {4, 5, 7},    {4, 5, 8},   {4, 6, 9},   {5, 7, 10}, {6, 8, 11},
    {6, 8, 13},  {7, 10, 14}, {8, 11, 16},  {9, 12, 18},  {10, 13, 20}, {11, 15, 23}, {13, 17, 25}};

struct DbParams {
    uint8_t* pl[3];      // picture being filtered in place
    const MbInfo* mb;
    int cw, ch, mbw, mbh;
    int alpha_y, beta_y, alpha_c, beta_c;
    int tc0_y[3], tc0_c[3];  // by bS-1
    SliceRows sl;        // several slices: disable_deblocking_filter_idc 2, the edge between two slices is left alone
    const uint8_t* bs;   // boundary strengths of k_bs / k_dec_bs_pos, 32 per macroblock: [dir][edge][segment]; the diagonal form reads these bytes, the persistent forms the same array as words (DbRowParams::bs)
    // k_deblock_rows<.., PERMB = true> (decoder peer): thresholds per edge from the two macroblocks' own QPs (8.7.2.2)
    const uint8_t* mbqp; // QP_Y per macroblock (0 for I_PCM)
    int oa, ob;          // FilterOffsetA, FilterOffsetB
    int cqo_cb, cqo_cr;  // chroma_qp_index_offset, second_chroma_qp_index_offset
};

// filter one line across an edge; p points at q0 inside LDS, xs = distance between samples across the edge
__device__ __forceinline__ void filter_line(uint8_t* pix, int xs, int bS, int alpha, int beta, int tc0, bool chroma)
{
    const int p0 = pix[-xs], p1 = pix[-2 * xs], q0 = pix[0], q1 = pix[xs];
    if (iabs(p0 - q0) >= alpha || iabs(p1 - p0) >= beta || iabs(q1 - q0) >= beta) return;
    if (chroma) {
        if (bS < 4) {
            const int tc = tc0 + 1;
            const int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
            pix[-xs] = (uint8_t)clip255(p0 + d);
            pix[0] = (uint8_t)clip255(q0 - d);
        } else {
            pix[-xs] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
            pix[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
        }
        return;
    }
    const int p2 = pix[-3 * xs], q2 = pix[2 * xs];
    const int ap = iabs(p2 - p0), aq = iabs(q2 - q0);
    if (bS < 4) {
        const int tc = tc0 + (ap < beta) + (aq < beta);
        const int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
        pix[-xs] = (uint8_t)clip255(p0 + d);
        pix[0] = (uint8_t)clip255(q0 - d);
        if (ap < beta) pix[-2 * xs] = (uint8_t)(p1 + clip3(-tc0, tc0, (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1));
        if (aq < beta) pix[xs] = (uint8_t)(q1 + clip3(-tc0, tc0, (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1));
    } else {
        const int p3 = pix[-4 * xs], q3 = pix[3 * xs];
        const bool strong = iabs(p0 - q0) < ((alpha >> 2) + 2);
        if (ap < beta && strong) {
            pix[-xs] = (uint8_t)((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3);
            pix[-2 * xs] = (uint8_t)((p2 + p1 + p0 + q0 + 2) >> 2);
            pix[-3 * xs] = (uint8_t)((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3);
        } else pix[-xs] = (uint8_t)((2 * p1 + p0 + q1 + 2) >> 2);
        if (aq < beta && strong) {
            pix[0] = (uint8_t)((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3);
            pix[xs] = (uint8_t)((p0 + q0 + q1 + q2 + 2) >> 2);
            pix[2 * xs] = (uint8_t)((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3);
        } else pix[0] = (uint8_t)((2 * q1 + q0 + p1 + 2) >> 2);
    }
}

enum { DB_LP = 24, DB_CP = 12 };  // LDS pitches: luma 20 wide, chroma 10 wide (4 / 2 apron)

__global__ __launch_bounds__(64) void k_deblock_diag(DbParams D, int s)
{   // (single-item debug form: no batch dimension)
    const int lane = threadIdx.x;
    // macroblocks with mx + 2*my == s
    const int ymin = max(0, (s - (D.mbw - 1) + 1) >> 1);
    const int my = ymin + blockIdx.x, mx = s - 2 * my;
    if (my >= D.mbh || mx < 0 || mx >= D.mbw) return;
    const int cs = D.cw / 2;
    __shared__ __attribute__((aligned(16))) uint8_t s_y[20 * DB_LP];      // rows/cols -4..15
    __shared__ __attribute__((aligned(16))) uint8_t s_c[2][10 * DB_CP];   // rows/cols -2..7
    __shared__ uint8_t s_bs[2][16];  // [dir][edge*4 + segment]

    // load 20x20 luma (as 5 dwords per row) and 10x10 chroma; out-of-picture apron left as is (never filtered)
    for (int i = lane; i < 20 * 5; i += 64) {
        const int r = i / 5, c = i - r * 5;
        const int gy = 16 * my - 4 + r, gx = 16 * mx - 4 + c * 4;
        uint32_t v = 0;
        if (gy >= 0 && gx >= 0) v = *(const uint32_t*)(D.pl[0] + (size_t)gy * D.cw + gx);
        *(uint32_t*)(s_y + r * DB_LP + c * 4) = v;
    }
    for (int i = lane; i < 2 * 10 * 5; i += 64) {
        const int pl = i / 50, k = i - pl * 50, r = k / 5, c = k - r * 5;
        const int gy = 8 * my - 2 + r, gx = 8 * mx - 2 + c * 2;
        uint16_t v = 0;
        if (gy >= 0 && gx >= 0) v = *(const uint16_t*)(D.pl[1 + pl] + (size_t)gy * cs + gx);
        *(uint16_t*)(s_c[pl] + r * DB_CP + c * 2) = v;
    }
    if (lane < 32) {
        const int dir = lane >> 4, e = (lane >> 2) & 3, k = lane & 3;  // k: segment along the edge
        const int bS = D.bs[((size_t)my * D.mbw + mx) * 32 + lane];   // k_bs (k_cavlc.h mb_edge_strength), same (dir, edge, segment) order
        s_bs[dir][e * 4 + k] = (uint8_t)bS;
    }
    __syncthreads();

    // lanes 0..15: luma lines; 16..23: Cb lines; 24..31: Cr lines
    const bool isY = lane < 16, isC = lane >= 16 && lane < 32;
    const int cpl = (lane >> 3) & 1, cl = lane & 7;
#pragma unroll 1
    for (int dir = 0; dir < 2; dir++) {
#pragma unroll 1
        for (int e = 0; e < 4; e++) {
            if (isY) {
                const int bS = s_bs[dir][e * 4 + (lane >> 2)];
                if (bS) {
                    uint8_t* p = dir == 0 ? s_y + (4 + lane) * DB_LP + 4 + 4 * e : s_y + (4 + 4 * e) * DB_LP + 4 + lane;
                    filter_line(p, dir == 0 ? 1 : DB_LP, bS, D.alpha_y, D.beta_y, bS < 4 ? D.tc0_y[bS - 1] : 0, false);
                }
            } else if (isC && !(e & 1)) {
                const int bS = s_bs[dir][e * 4 + (cl >> 1)];
                if (bS) {
                    uint8_t* p = dir == 0 ? s_c[cpl] + (2 + cl) * DB_CP + 2 + 2 * e : s_c[cpl] + (2 + 2 * e) * DB_CP + 2 + cl;
                    filter_line(p, dir == 0 ? 1 : DB_CP, bS, D.alpha_c, D.beta_c, bS < 4 ? D.tc0_c[bS - 1] : 0, true);
                }
            }
            __syncthreads();
        }
    }
    // write back: own block plus the 3 (luma) / 1 (chroma) neighbour columns and rows that may have changed.
    // 20x20 region minus the untouched first row/column of the apron; corner apron samples are never
    // modified by this macroblock and belong to other macroblocks, so they are skipped.
    for (int i = lane; i < 20 * 5; i += 64) {
        const int r = i / 5, c = i - r * 5;
        const int gy = 16 * my - 4 + r, gx = 16 * mx - 4 + c * 4;
        if (gy < 0 || gx < 0) continue;
        if (r < 4 && c == 0) continue;  // top-left corner block: not ours
        *(uint32_t*)(D.pl[0] + (size_t)gy * D.cw + gx) = *(const uint32_t*)(s_y + r * DB_LP + c * 4);
    }
    for (int i = lane; i < 2 * 10 * 5; i += 64) {
        const int pl = i / 50, k = i - pl * 50, r = k / 5, c = k - r * 5;
        const int gy = 8 * my - 2 + r, gx = 8 * mx - 2 + c * 2;
        if (gy < 0 || gx < 0) continue;
        if (r < 2 && c == 0) continue;
        *(uint16_t*)(D.pl[1 + pl] + (size_t)gy * cs + gx) = *(const uint16_t*)(s_c[pl] + r * DB_CP + c * 2);
    }
}

// ===========================================================================
// Persistent form: ONE launch, one wavefront per macroblock row.  Row r walks its
// macroblocks left to right; the HORIZONTAL edges of macroblock mx need the bottom
// four luma / two chroma sample rows of macroblock (mx, r-1), which row r-1
// PUBLISHES as soon as it has filtered the LEFT edge of macroblock mx+1 (the last
// thing that touches them: its columns 13..15).  The vertical edges of (mx, r)
// touch rows 0..15 of their own row only, so row r waits BETWEEN its two phases,
// not before the first.  That is the 8.7 raster-order dependency (left, top,
// top-right) and no more: a row runs about three quarters of a macroblock step
// plus the hand-off latency behind the one above it.
//
// Hand-off (cdna_hip_programming.md Guideline 16, form R2 "the data is the flag"):
// 24 granules per macroblock, each ONE aligned 8-byte agent-scope relaxed atomic
// store of {tag = picture serial, 4 samples}; the consumer re-reads its granules
// with agent-scope atomic loads (L1-bypassing) until every tag matches.  No fence,
// no separate flag, no drain.  Each sample of the picture has at most one writer:
// a row stores rows 0..11 of its macroblocks (0..5 chroma), the row below stores
// rows 12..15 (6..7) after its own top-edge filter - where it filters that edge;
// where it does not, nothing is handed down or waited for and the row stores all
// 16 itself, as the last row does everywhere.  A macroblock the filter cannot have
// changed is not stored at all (db_hands_down, db_dirty further down).
// Everything a macroblock needs from HBM (its samples, MbInfo, granules) is
// requested one macroblock ahead, so an iteration is LDS/VALU work only.
// Every spin is bounded; a timeout sets *err and the grid still drains.
// ===========================================================================
typedef unsigned long long u64;
#define AT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define AT_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct DbRowParams {
    DbParams d;
    u64* handoff;        // [mbh][mbw][24] granules: 16 luma dwords (rows 12..15), 8 chroma dwords (rows 6..7 of Cb, Cr)
    const uint32_t* bs;  // [nmb][8]: d.bs as words, word dir*4+edge, byte = segment along the edge
    unsigned* err;
    unsigned serial;     // changes every picture, never 0
    const unsigned* anybs;   // [item] == serial when the picture has any non-zero boundary strength (k_bs)
    const unsigned* anypcm;  // [item] == pic_serial: the picture holds an I_PCM macroblock and is not filtered (slice header idc 1)
    const unsigned* anyintra;   // [item] == pic_serial: a P picture with intra macroblocks (bS 3 / 4 edges)
    unsigned pic_serial;
    int npic;                // pictures of the step (gridDim.y of them at a time)
    int need_intra;          // the stream hub and decoder groups launch P steps in both forms: < 0 this form runs when the picture
                             // has no intra macroblock, > 0 when it has; 0 = unconditional (IDR steps, and k_deblock_*_p which
                             // choose the form themselves)
    // lockstep batch strides (gridDim.y items)
    size_t st_y, st_c, st_handoff;   // bytes, bytes, u64 words
    int st_mb;
    int row0;            // first macroblock row of this instance's band (blockIdx.x counts from it)
    // indirect launches (IND = true, dev_common.h item_ref): position -> item, its ring slot and its QP; d.pl[] = plane bases
    const uint32_t* itemtab;
    size_t st_ring_y, st_ring_c;
    const DecPos* dectab;    // decoder groups (PERMB): position -> what the picture has of its own (dev_common.h)
};

// One edge, one line of samples held in registers, branch-free so that luma and
// chroma lines share one instruction stream (8.7.2.3 / 8.7.2.4).  chroma lanes
// never touch p1/q1 and use tc = tc0 + 1.  BS4 compiles the intra (bS = 4) form in.
template <bool BS4>
__device__ __forceinline__ void filt_uni(const int p3, int& p2, int& p1, int& p0, int& q0, int& q1, int& q2, const int q3,
                                         int bS, bool chroma, int alpha, int beta, int t1, int t2, int t3)
{
    // Every decision is an all-ones / all-zero MASK applied with AND, not a select: hipcc turns chains of selects over
    // this much arithmetic back into exec-masked regions with branches, and on a wave that runs alone on its SIMD
    // every s_and_saveexec / s_cbranch pair is dead time in the dependency chain.
    const int tc0 = bS == 1 ? t1 : (bS == 2 ? t2 : t3);
    const int fm = -(int)(bS != 0 && iabs(p0 - q0) < alpha && iabs(p1 - p0) < beta && iabs(q1 - q0) < beta);
    const int lum = chroma ? 0 : -1;
    const int apm = lum & -(int)(iabs(p2 - p0) < beta), aqm = lum & -(int)(iabs(q2 - q0) < beta);
    const int tc = tc0 + (chroma ? 1 : 0) - apm - aqm;          // + 1 per true luma condition
    const int d = clip3(-tc, tc, (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3);
    const int avg = (p0 + q0 + 1) >> 1;
    int dp0 = clip255(p0 + d) - p0, dq0 = clip255(q0 - d) - q0;                 // changes of the normal filter
    int dp1 = apm & clip3(-tc0, tc0, (p2 + avg - (p1 << 1)) >> 1);
    int dq1 = aqm & clip3(-tc0, tc0, (q2 + avg - (q1 << 1)) >> 1);
    int dp2 = 0, dq2 = 0;
    if (BS4) {
        const int s4 = -(int)(bS == 4);
        const int strong = -(int)(iabs(p0 - q0) < ((alpha >> 2) + 2));
        const int sp = apm & strong, sq = aqm & strong;
        // strong (8.7.2.4) and weak intra forms as changes; sp / sq pick per side
        const int wp0 = (sp & (((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3) - p0)) | (~sp & (((2 * p1 + p0 + q1 + 2) >> 2) - p0));
        const int wq0 = (sq & (((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3) - q0)) | (~sq & (((2 * q1 + q0 + p1 + 2) >> 2) - q0));
        const int wp1 = sp & (((p2 + p1 + p0 + q0 + 2) >> 2) - p1), wq1 = sq & (((p0 + q0 + q1 + q2 + 2) >> 2) - q1);
        const int wp2 = sp & (((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3) - p2), wq2 = sq & (((2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3) - q2);
        dp0 = (s4 & wp0) | (~s4 & dp0); dq0 = (s4 & wq0) | (~s4 & dq0);
        dp1 = (s4 & wp1) | (~s4 & dp1); dq1 = (s4 & wq1) | (~s4 & dq1);
        dp2 = s4 & wp2; dq2 = s4 & wq2;
    }
    p0 += fm & dp0; q0 += fm & dq0; p1 += fm & dp1; q1 += fm & dq1;
    if (BS4) { p2 += fm & dp2; q2 += fm & dq2; }
}

enum { DR_LP = 40, DR_CP = 24 };  // LDS pitches; luma tile cols -16..15 (+4 pad), rows -4..15; chroma cols -8..7, rows -4..15
// One tile holds luma and both chroma planes at offsets chosen for the LDS banks (64 x 4 B; ds_read / write_b32 serve 32 lanes at
// a time by (address / 4) mod 32).  The vertical-edge phase has 16 luma and 16 chroma lanes each read and write dword w of ITS
// line: luma lines are 10 dwords apart and take the 16 banks of one parity; chroma lines 6 dwords apart take 8 banks of the other
// parity when the plane starts at an odd dword (DR_CB), and the second plane the remaining 8 when it lies 16 mod 32 dwords
// after the first (DR_CPS) - 32 lanes, 32 banks.  (Separate arrays had put all 32 lines on the 16 odd banks, the two chroma
// planes partly on each other's: 2- and 3-way conflicts on every access of the phase)
enum { DR_CB = 4 * 201, DR_CPS = 4 * 144, DR_TILE = DR_CB + 2 * DR_CPS + 12 };
enum { DR_PAIR_TILE = (DR_TILE + 127) / 128 * 128 };   // the pair form's two tiles lie a multiple of 32 dwords apart: the same banks
// sample (r, c) of a tile's luma / of its chroma plane pl; (0, 0) = first sample of the current macroblock, the previous one to its left
__device__ __forceinline__ uint8_t* db_y(uint8_t* const tile, const int r, const int c) { return tile + (r + 4) * DR_LP + c + 16; }
__device__ __forceinline__ uint8_t* db_c(uint8_t* const tile, const int pl, const int r, const int c) { return tile + DR_CB + pl * DR_CPS + (r + 4) * DR_CP + c + 8; }
__device__ __forceinline__ uint32_t& dw(uint8_t* const p) { return *(uint32_t*)p; }   // the aligned dword at p

// The steps of a macroblock, once for both persistent forms.  A form keeps what is its own - which lanes move the samples, where
// the bottom rows go, the prefetch, the order of the steps and their wave_sync() points - and calls these for the rest.
struct DbThr { int al, be, t1, t2, t3; };   // alpha, beta and tc0 by bS 1..3 of one edge, luma or chroma as the lane's line
__device__ __forceinline__ DbThr db_picture_thr(const DbParams& D, const bool isC)
{
    return isC ? DbThr{D.alpha_c, D.beta_c, D.tc0_c[0], D.tc0_c[1], D.tc0_c[2]} : DbThr{D.alpha_y, D.beta_y, D.tc0_y[0], D.tc0_y[1], D.tc0_y[2]};
}
// The picture at position pos of the step (blockIdx.y, or the one this workgroup walks to).  false: this launch has nothing to do
// on it and nobody waits.  Otherwise D is R.d moved to the picture (planes, macroblock records; IND: ring slot and thresholds)
template <bool PERMB, bool IND>
__device__ __forceinline__ bool db_picture_view(const DbRowParams& R, const int pos, DbParams& D, u64*& handoff, const uint32_t*& bsw)
{
    if constexpr (PERMB) {
        // decoder groups: the position is a row of the decoder table (dev_common.h DecPos): item, ring slot, filter offsets, chroma QP
        // offsets and the filter's slice bands are the picture's own; the thresholds come per edge from mbqp.  need_intra picks the
        // form by the table's flag (a decoder's I_PCM macroblocks never switch the filter off: anypcm is not looked at)
        const DecPosRef dp = dec_pos(R.dectab, pos);
        if (!dp.filtered || R.anybs[dp.item] != R.serial) return false;
        if (R.need_intra != 0 && dp.intra != (R.need_intra > 0)) return false;
        D = R.d;
        const size_t g = (size_t)dp.item;
        D.pl[0] += g * R.st_y + (size_t)dp.cur * R.st_ring_y; D.pl[1] += g * R.st_c + (size_t)dp.cur * R.st_ring_c; D.pl[2] += g * R.st_c + (size_t)dp.cur * R.st_ring_c;
        D.mb += g * R.st_mb; D.mbqp += g * R.st_mb;
        D.oa = dp.oa; D.ob = dp.ob; D.cqo_cb = dp.cqo_cb; D.cqo_cr = dp.cqo_cr; D.sl = dp.fsl;
        handoff = R.handoff + g * R.st_handoff;
        bsw = R.bs + g * R.st_mb * 8;
        return true;
    } else {
    const int bitem = batch_item<IND>(R.itemtab, pos);
    if (R.anybs[bitem] != R.serial) return false;   // no edge of this picture is filtered
    if (R.anypcm[bitem] == R.pic_serial) return false;
    if (R.need_intra != 0 && (R.anyintra[bitem] == R.pic_serial) != (R.need_intra > 0)) return false;
    D = R.d;
    const size_t g = (size_t)bitem;
    D.pl[0] += g * R.st_y; D.pl[1] += g * R.st_c; D.pl[2] += g * R.st_c; D.mb += g * R.st_mb;
    if constexpr (IND) {   // the item's own ring slot and its own QP's thresholds (Tables 8-16 / 8-17, chroma through Table 8-15)
        const ItemRef it = item_ref(R.itemtab, pos);
        D.pl[0] += (size_t)it.cur * R.st_ring_y; D.pl[1] += (size_t)it.cur * R.st_ring_c; D.pl[2] += (size_t)it.cur * R.st_ring_c;
        const int qpc = c_chroma_qp[it.qp];
        D.alpha_y = c_alpha[it.qp]; D.beta_y = c_beta[it.qp]; D.alpha_c = c_alpha[qpc]; D.beta_c = c_beta[qpc];
#pragma unroll
        for (int i = 0; i < 3; i++) { D.tc0_y[i] = c_tc0[it.qp][i]; D.tc0_c[i] = c_tc0[qpc][i]; }
    }
    handoff = R.handoff + g * R.st_handoff;
    bsw = R.bs + g * R.st_mb * 8;
    return true;
    }
}
// Filter lane l of a row: 0..15 the luma lines, 16..31 the chroma lines (plane fpl, line).  V phase: the lane holds line fln of
// its plane (vrow: 4-byte aligned, from column -4), H phase: column fln (hcol: from row -4).  seg8: shift to its segment's strength
struct DbLane { bool isC; int fpl, seg8, hstride; uint8_t *vrow, *hcol; };
__device__ __forceinline__ DbLane db_lane(const int l, uint8_t* const tile)
{
    DbLane L;
    L.isC = l >= 16; L.fpl = (l >> 3) & 1;
    const int fln = L.isC ? (l & 7) : l;
    L.seg8 = 8 * (L.isC ? (fln >> 1) : (fln >> 2));
    L.vrow = L.isC ? db_c(tile, L.fpl, fln, -4) : db_y(tile, fln, -4);
    L.hcol = L.isC ? db_c(tile, L.fpl, -4, fln) : db_y(tile, -4, fln);
    L.hstride = L.isC ? DR_CP : DR_LP;
    return L;
}
// Edge E (0..3) of one direction on the line px[]: b = that direction's four strength words (byte = segment along the edge).
// Chroma lines have edges 0 and 1 only, which are luma edges 0 and 2.  An edge no line of which is filtered (bS 0 in every
// segment, luma and chroma: three of four inner edges on ordinary P pictures) is skipped by ONE wave-uniform branch - not a
// branch inside the filter, see filt_uni.  Returns whether the edge was filtered.
template <bool BS4, int E>
__device__ __forceinline__ bool db_edge(const DbLane& L, int (&px)[20], const uint4 b, const DbThr& T)
{
    const uint32_t w = E == 0 ? b.x : E == 1 ? (L.isC ? b.z : b.y) : E == 2 ? b.z : b.w;
    const int bS = (E >= 2 && L.isC) ? 0 : (int)((w >> L.seg8) & 255);
    if (__ballot(bS != 0) == 0ull) return false;
    filt_uni<BS4>(px[4 * E], px[4 * E + 1], px[4 * E + 2], px[4 * E + 3], px[4 * E + 4], px[4 * E + 5], px[4 * E + 6], px[4 * E + 7],
                  bS, L.isC, T.al, T.be, T.t1, T.t2, T.t3);
    return true;
}
template <int W>
__device__ __forceinline__ uint32_t db_pack(const int (&px)[20])   // dword W of the line
{
    return (uint32_t)px[4 * W] | ((uint32_t)px[4 * W + 1] << 8) | ((uint32_t)px[4 * W + 2] << 16) | ((uint32_t)px[4 * W + 3] << 24);
}
// Vertical edges: lane = one line of samples, four edges in registers (px[] is the caller's: it lives across the publish).  The
// left edge goes first and its p side (the one tile dword of the previous macroblock it can change) is written back at once:
// the previous macroblock is final from here, and the row below is waiting for it.  Then edges 1..3 from the same registers.
template <bool BS4>
__device__ __forceinline__ void db_left_edge(const DbLane& L, int (&px)[20], const uint4 b0, const bool on, const DbThr& T)
{
    if (on) {
#pragma unroll
        for (int w = 0; w < 5; w++) {
            const uint32_t v = dw(L.vrow + 4 * w);
#pragma unroll
            for (int b = 0; b < 4; b++) px[4 * w + b] = (int)((v >> (8 * b)) & 255);
        }
        if (db_edge<BS4, 0>(L, px, b0, T)) dw(L.vrow) = db_pack<0>(px);
    }
}
template <bool BS4>
__device__ __forceinline__ void db_inner_vertical(const DbLane& L, int (&px)[20], const uint4 b0, const bool on, const DbThr& T)
{
    if (on) {
        db_edge<BS4, 1>(L, px, b0, T);
        db_edge<BS4, 2>(L, px, b0, T);
        db_edge<BS4, 3>(L, px, b0, T);
        dw(L.vrow + 4) = db_pack<1>(px); dw(L.vrow + 8) = db_pack<2>(px);
        if (!L.isC) { dw(L.vrow + 12) = db_pack<3>(px); dw(L.vrow + 16) = db_pack<4>(px); }
    }
}
// Horizontal edges: lane = one column of samples (rows -4..15; chroma uses rows -4..7 of its tile); Ttop: the edge to the macroblock above
template <bool BS4>
__device__ __forceinline__ void db_horizontal(const DbLane& L, const uint4 b1, const bool on, const DbThr& Ttop, const DbThr& T)
{
    if (on) {
        int px[20];
#pragma unroll
        for (int r = 0; r < 20; r++) px[r] = L.hcol[r * L.hstride];
        db_edge<BS4, 0>(L, px, b1, Ttop);
        db_edge<BS4, 1>(L, px, b1, T);
        db_edge<BS4, 2>(L, px, b1, T);
        db_edge<BS4, 3>(L, px, b1, T);
        // samples an edge can change: p2..q2 around rows 0,4,8,12 -> rows -3..14; chroma: p0,q0 around rows 0,4
#pragma unroll
        for (int r = 1; r < 19; r++) {
            const bool both = r == 3 || r == 4 || r == 7 || r == 8;
            if (both || !L.isC) L.hcol[r * L.hstride] = (uint8_t)px[r];
        }
    }
}
// Granule k of a macroblock, one dword of its bottom sample rows: f(chroma, plane, row, byte column), position in the macroblock.
// 0..15: luma row 12 + k/4, dword k%4; 16..23: chroma plane (k-16)/4, row 6 + ((k-16)/2)%2, dword (k-16)%2; lanes k >= 24 have none.
template <class F>
__device__ __forceinline__ void db_granule(const int k, F f)
{
    if (k < 16) f(false, 0, 12 + (k >> 2), (k & 3) * 4);
    else if (k < 24) f(true, (k - 16) >> 2, 6 + (((k - 16) >> 1) & 1), ((k - 16) & 1) * 4);
}
// that position in the tile, in the macroblock (dmx, dmy) from the current one
__device__ __forceinline__ uint8_t* db_tile_at(uint8_t* const tile, const bool c, const int pl, const int r, const int col, const int dmx, const int dmy)
{
    return c ? db_c(tile, pl, 8 * dmy + r, 8 * dmx + col) : db_y(tile, 16 * dmy + r, 16 * dmx + col);
}
// bottom dword k of the previous macroblock (shifted: it lies to the left of the current one) or of the current one
__device__ __forceinline__ uint32_t db_bottom_dword(uint8_t* const tile, const int k, const bool shifted)
{
    uint32_t v = 0;
    db_granule(k, [&](bool c, int pl, int r, int col) { v = dw(db_tile_at(tile, c, pl, r, col, shifted ? -1 : 0, 0)); });
    return v;
}
// dword k of the macroblock above: into the tile's top apron, and from there (filtered, final) to the picture
__device__ __forceinline__ void db_put_apron(uint8_t* const tile, const int k, const uint32_t v)
{
    db_granule(k, [&](bool c, int pl, int r, int col) { dw(db_tile_at(tile, c, pl, r, col, 0, -1)) = v; });
}
__device__ __forceinline__ void db_store_apron(const DbParams& D, uint8_t* const tile, const int k, const int mx, const int my)
{
    db_granule(k, [&](bool c, int pl, int r, int col) {
        uint8_t* const p = c ? (pl ? D.pl[2] : D.pl[1]) + (size_t)(8 * (my - 1) + r) * (D.cw / 2) + 8 * mx + col
                             : D.pl[0] + (size_t)(16 * (my - 1) + r) * D.cw + 16 * mx + col;
        dw(p) = dw(db_tile_at(tile, c, pl, r, col, 0, -1));
    });
}
// -DDB_AB_COUNT (measurement build, make ab): what the macroblock steps wait on.  Per wave in registers, added once at the wave's
// end with vector atomic adds: iterations that have a wait, those whose prefetched tag was stale, those still stale at the first
// look (the same number since the re-request left), spin passes.  The host reads and clears the four words with mi355x_h264_db_counts().
// Since the sparse hand-off four more.  Three are counted per row (a wave of the pair form counts each of its rows; lanes 0 and 32
// add) and are the picture's own, whatever the form: macroblocks with a filtered top edge (an apron to take, through LDS or after a
// wait), macroblocks whose stores were skipped (clean), sets of bottom rows handed down (granules or ring slots).  The fourth is the
// wave's: iterations in which no row of the wave has an edge to filter, a macroblock to store or rows to hand down (the row form
// counts its macroblock iterations, the pair form all of them).  mi355x_h264_db_counts2() reads all eight; tools/db_sparsity.py
// restates them from the oracle's macroblock records.
struct DbCount { unsigned iters, stale, still_stale, spins, top_on, idle, skipped, published; };
#define DB_COUNT_ZERO {0, 0, 0, 0, 0, 0, 0, 0}
#ifdef DB_AB_COUNT
__device__ unsigned g_db_count[8];
__device__ __forceinline__ void db_count_flush(const DbCount& c, const int lane, const bool two_rows)
{
    if (lane == 0 && c.iters) {
        atomicAdd(&g_db_count[0], c.iters); atomicAdd(&g_db_count[1], c.stale);
        atomicAdd(&g_db_count[2], c.still_stale); atomicAdd(&g_db_count[3], c.spins);
    }
    if (lane == 0) atomicAdd(&g_db_count[5], c.idle);
    if (lane == 0 || (two_rows && lane == 32)) {
        atomicAdd(&g_db_count[4], c.top_on); atomicAdd(&g_db_count[6], c.skipped); atomicAdd(&g_db_count[7], c.published);
    }
}
}  // namespace h264
extern "C" __attribute__((visibility("default"))) int mi355x_h264_db_counts(unsigned out[4], int clear)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(h264::g_db_count), 4 * sizeof(unsigned)) != hipSuccess) return -1;
    const unsigned zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // (all eight: one set of counters)
    if (clear && hipMemcpyToSymbol(HIP_SYMBOL(h264::g_db_count), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
extern "C" __attribute__((visibility("default"))) int mi355x_h264_db_counts2(unsigned out[8], int clear)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(h264::g_db_count), 8 * sizeof(unsigned)) != hipSuccess) return -1;
    const unsigned zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (clear && hipMemcpyToSymbol(HIP_SYMBOL(h264::g_db_count), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
namespace h264 {
#define DB_COUNT(x) x
#else
#define DB_COUNT(x)
#endif
// Wait until the granule g of every lane that needs one carries this picture's tag, re-reading it from addr.  The FIRST look
// stands in front of the spin and is at the prefetched copy, which consume() has waited for an iteration ago: a wave whose
// granules came fresh reaches the horizontal edges without any wait for memory - in particular without the one for this
// iteration's own publish, whose write-through stores were issued a few dozen instructions earlier (a spin loop that starts
// with the compare gets s_waitcnt vmcnt(0) at its head, because g may come from the reload, and every wave ran into it in
// every iteration).  Only a wave that has to spin waits for everything (the reload's vmcnt(0)), and it is waiting anyway.
// Bounded: a timeout sets timed_out, and no later wait of the wave spins at all.
// (Asking again for a stale granule at the top of the iteration, ahead of the vertical edges, was measured beside this and
// dropped: DESIGN.md section 11.)
__device__ __forceinline__ void db_wait_tags(const bool need, u64& g, const u64* const addr, const unsigned serial, bool& timed_out, DbCount& cnt)
{
    const bool stale = __ballot(need && (unsigned)(g >> 32) != serial) != 0ull;
    DB_COUNT(if (__ballot(need) != 0ull) { cnt.iters++; if (stale) { cnt.stale++; cnt.still_stale++; } })
    if (timed_out || !stale) return;
    unsigned spins = 0;
    do {
        if (++spins > (1u << 20)) { timed_out = true; break; }
        __builtin_amdgcn_s_sleep(1);
        if (need) g = AT_LOAD(addr);
    } while (__ballot(need && (unsigned)(g >> 32) != serial) != 0ull);
    DB_COUNT(cnt.spins += spins;)
}
// The hand-off and the stores happen only where the picture needs them.  Both tests are uniform over the lanes of a row.
//   db_hands_down: macroblock (x, r) hands its bottom rows (12..15 / 6..7) to the row below exactly where that row filters its top
//     edge there: below_top = bS word (dir 1, edge 0) of macroblock (x, r + 1), any segment.  The row below decides its wait, its top
//     apron and the apron's store by the SAME word of the SAME array (its own b1.x), which k_bs / k_dec_bs_pos wrote before the
//     launch: a wait exists only where a publish does.  Elsewhere row r stores the rows itself, and db_horizontal with edge 0
//     skipped (or run with bS 0 beside the pair's other row: no sample changes) makes no use of tile rows -4..-1.
//   db_dirty: a macroblock's samples can differ from the picture's - the filter works in place - only when one of its own eight
//     edge groups has a strength, or the left edge of its right neighbour (nb0; none behind the last macroblock), or the top edge
//     below (then the rows it can change travel down and are stored there).  A clean macroblock stores nothing.  A strength whose
//     alpha / beta test fails on every line still counts as dirty: conservative, and known without looking at a sample.
// SAFETY of the sparse hand-off: the set of waits is a subset of the waits of the form that handed every macroblock down; every
// wait that remains is answered by a publish decided from the same memory word; there is no new spin and no fence, and the bounded
// spin with its timed_out path (db_wait_tags) is as it was.  Every sample of the picture keeps at most one writer.
__device__ __forceinline__ bool db_hands_down(const bool last_row, const uint32_t below_top) { return !last_row && below_top != 0; }
__device__ __forceinline__ bool db_dirty(const uint32_t own, const bool have_right, const uint4 nb0) { return own != 0 || (have_right && nb0.x != 0); }
__device__ __forceinline__ uint32_t db_any(const uint4 b0, const uint4 b1) { return b0.x | b0.y | b0.z | b0.w | b1.x | b1.y | b1.z | b1.w; }

// ===========================================================================
// Row form: one wave per macroblock row; all 64 lanes move samples (one luma dword each), lanes 0..31 filter.
// PERMB (the decoder peer, streams of other encoders): qPp / qPq are the two macroblocks' own QPs (mb_qp_delta, I_PCM = 0),
// the chroma QPs go through chroma_qp_index_offset, indexA / indexB through the slice's filter offsets - three threshold
// sets per macroblock (left edge, top edge, inner edges), looked up in LDS copies of Tables 8-15 / 8-16.  PERMB = false is
// the encoder's form: one set per picture, prepared on the host.
// ===========================================================================
template <bool BS4, bool PERMB, bool IND>
__device__ __forceinline__ void deblock_rows_picture(const DbRowParams& R, const int pos, const int lane, uint8_t* const s_y)
{
    DbParams D; u64* handoff; const uint32_t* bsw;
    if (!db_picture_view<PERMB, IND>(R, pos, D, handoff, bsw)) return;
    const int my = R.row0 + blockIdx.x, cs = D.cw / 2;   // (row0: first row of this instance's band)
    // a slice's rows form a wavefront of their own: its first row waits for nobody (no edge to the slice above is
    // filtered), its last row stores all sixteen sample rows itself
    const bool first_row = !D.sl.has_top(my);
    const bool last_row = my == D.mbh - 1 || !D.sl.has_top(my + 1);
    bool timed_out = false;
    const int yr = lane >> 2, yc4 = (lane & 3) * 4;                                   // luma dword owned by this lane
    const int cpl_l = (lane >> 4) & 1, cr_l = (lane >> 1) & 7, cc4 = (lane & 1) * 4;  // chroma dword (lanes < 32)
    const DbLane L = db_lane(lane, s_y);   // (lanes 32..63 get a role too and never act in it)
    // thresholds of the inner edges, of the left edge (L) and of the top edge (T); one set unless PERMB
    DbThr thr = db_picture_thr(D, L.isC), thrL = thr, thrT = thr;
    __shared__ uint32_t s_tA[PERMB ? 52 : 1];   // by indexA: alpha << 24 | tc0(bS 3) << 16 | tc0(bS 2) << 8 | tc0(bS 1)
    __shared__ uint8_t s_tB[PERMB ? 52 : 1], s_cq[PERMB ? 52 : 1];   // beta by indexB; QP_C by the offset luma QP
    if (PERMB) {
        if (lane < 52) {
            s_tA[lane] = ((uint32_t)c_alpha[lane] << 24) | ((uint32_t)c_tc0[lane][2] << 16) | ((uint32_t)c_tc0[lane][1] << 8) | (uint32_t)c_tc0[lane][0];
            s_tB[lane] = c_beta[lane];
            s_cq[lane] = c_chroma_qp[lane];
        }
        wave_sync();
    }
    const int cqo = L.fpl ? D.cqo_cr : D.cqo_cb;
    auto thresholds = [&](const int qa, const int qb) {
        const int ca = (int)s_cq[clip3(0, 51, qa + cqo)], cb = (int)s_cq[clip3(0, 51, qb + cqo)];
        const int av = ((L.isC ? ca : qa) + (L.isC ? cb : qb) + 1) >> 1;           // qPav (8-461)
        const uint32_t w = s_tA[clip3(0, 51, av + D.oa)];
        return DbThr{(int)(w >> 24), (int)s_tB[clip3(0, 51, av + D.ob)], (int)(w & 255u), (int)((w >> 8) & 255u), (int)((w >> 16) & 255u)};
    };
    uint32_t pf_q = 0;   // QP_Y of the macroblock | of the one above << 8
    int qp_left = 0;

    // Software pipeline: the samples, boundary strengths and hand-off granules of macroblock mx+1 are
    // requested (straight-line, unconditional loads; past the end of the row the last macroblock's once more) after
    // macroblock mx has been put into LDS, and travel while mx is filtered.  vmcnt counts loads and stores together, in
    // order, and this iteration's publish is issued BEHIND them, between the vertical edges: so the one wait for memory in
    // front of the horizontal edges (db_wait_tags) looks at a copy of the granule that is older than the publish, and the
    // loads are collected after the horizontal edges (consume), by when the stores' acknowledgements have had that phase to
    // come back.  No macroblock step waits for its own stores unless it has to spin for the row above anyway.
    uint32_t pf_y = 0, pf_c = 0;
    uint4 pf_b0 = {0, 0, 0, 0}, pf_b1 = pf_b0;
    u64 pf_g = 0;
    uint32_t pf_tn = 0;   // top-edge strengths of the macroblock BELOW (its bS word dir 1, edge 0): does that row take our bottom rows?
    const int grow = first_row ? my : my - 1;      // a first row reads (and ignores) its own slots
    const int trow = last_row ? my : my + 1;       // (a last row hands nothing down and ignores the word)
    const int glane = lane < 24 ? lane : lane - 24 < 24 ? lane - 24 : lane - 48;
    const int last_mx = D.mbw - 1;
    auto prefetch = [&](int mx) {   // mx clamped by the caller into 0 .. mbw - 1
        pf_y = *(const uint32_t*)(D.pl[0] + (size_t)(16 * my + yr) * D.cw + 16 * mx + yc4);
        pf_c = *(const uint32_t*)((cpl_l ? D.pl[2] : D.pl[1]) + (size_t)(8 * my + cr_l) * cs + 8 * mx + cc4);   // lanes >= 32 mirror lanes < 32
        const uint4* b = (const uint4*)(bsw + ((size_t)my * D.mbw + mx) * 8);
        pf_b0 = b[0]; pf_b1 = b[1];
        pf_g = AT_LOAD(handoff + ((size_t)grow * D.mbw + mx) * 24 + glane);
        pf_tn = bsw[((size_t)trow * D.mbw + mx) * 8 + 4];
        if (PERMB) pf_q = (uint32_t)D.mbqp[(size_t)my * D.mbw + mx] | ((uint32_t)D.mbqp[(size_t)grow * D.mbw + mx] << 8);
    };
    auto consume = [&]() {   // forces the waits for the prefetched registers to sit here
        asm volatile("" : "+v"(pf_y), "+v"(pf_c), "+v"(pf_g), "+v"(pf_tn));
        asm volatile("" : "+v"(pf_b0.x), "+v"(pf_b0.y), "+v"(pf_b0.z), "+v"(pf_b0.w));
        asm volatile("" : "+v"(pf_b1.x), "+v"(pf_b1.y), "+v"(pf_b1.z), "+v"(pf_b1.w));
        if (PERMB) asm volatile("" : "+v"(pf_q));
    };
    prefetch(0);
    consume();
    uint32_t cur_y = pf_y, cur_c = pf_c, cur_q = pf_q;
    uint4 b0 = pf_b0, b1 = pf_b1;
    u64 g = pf_g;
    uint32_t tn = pf_tn, prev_tn = 0, prev_own = 0;   // prev_*: of macroblock mx - 1, which store_prev serves
    DbCount cnt = DB_COUNT_ZERO;

    // the previous macroblock is final with respect to this row once the current one's LEFT edge has been filtered (its
    // other vertical edges and its horizontal edges do not touch it): store / publish it.  Issued between the left edge and
    // edges 1..3, so that the row below gets it as early as 8.7 allows.  The stores' acknowledgements (the agent-scope
    // granule stores go all the way to the memory side; vmcnt retires in order) have edges 1..3 AND the horizontal edges to
    // come back: db_wait_tags between the two does not wait for them (see there), the next full wait is consume().
    auto store_prev = [&](const int mx, const bool have_cur) {
        if (mx > 0) {
            const int pmx = mx - 1;
            const int co = have_cur ? -16 : 0, cco = have_cur ? -8 : 0;  // after the last macroblock there was no shift
            const bool down = db_hands_down(last_row, prev_tn), dirty = db_dirty(prev_own, have_cur, b0);
            const int nrow = down ? 12 : 16, ncrow = down ? 6 : 8;
            DB_COUNT(if (!dirty) cnt.skipped++; if (down) cnt.published++;)
            if (dirty && yr < nrow) *(uint32_t*)(D.pl[0] + (size_t)(16 * my + yr) * D.cw + 16 * pmx + yc4) = dw(db_y(s_y, yr, co + yc4));
            if (dirty && lane < 32 && cr_l < ncrow)
                *(uint32_t*)((cpl_l ? D.pl[2] : D.pl[1]) + (size_t)(8 * my + cr_l) * cs + 8 * pmx + cc4) = dw(db_c(s_y, cpl_l, cr_l, cco + cc4));
            if (down && lane < 24)
                AT_STORE(handoff + ((size_t)my * D.mbw + pmx) * 24 + lane, ((u64)R.serial << 32) | db_bottom_dword(s_y, lane, have_cur));
        }
    };
    for (int mx = 0; mx <= D.mbw; mx++) {
        const bool have_cur = mx < D.mbw;
        if (have_cur) {
            // 1. previous macroblock moves to the left half of the tile
            if (mx > 0) {
                dw(db_y(s_y, yr, yc4 - 16)) = dw(db_y(s_y, yr, yc4));
                if (lane < 32) dw(db_c(s_y, cpl_l, cr_l, cc4 - 8)) = dw(db_c(s_y, cpl_l, cr_l, cc4));
            }
            wave_sync();
            // 2. current macroblock into LDS
            dw(db_y(s_y, yr, yc4)) = cur_y;
            if (lane < 32) dw(db_c(s_y, cpl_l, cr_l, cc4)) = cur_c;
            // requests for the next macroblock leave now and are collected after the filter (clamped: the same loads
            // whatever the position in the row; those of the last macroblock again are harmless)
            prefetch(mx + 1 > last_mx ? last_mx : mx + 1);
            if (PERMB) {
                const int qc = (int)(cur_q & 255u), qt = (int)(cur_q >> 8);
                thr = thresholds(qc, qc);
                thrL = thresholds(mx > 0 ? qp_left : qc, qc);
                thrT = thresholds(qt, qc);
                qp_left = qc;
            }
            wave_sync();
            const bool v_on = (b0.x | b0.y | b0.z | b0.w) != 0 && lane < 32, h_on = (b1.x | b1.y | b1.z | b1.w) != 0 && lane < 32;
            // 3. vertical edges, the left one first
            int px[20];
            db_left_edge<BS4>(L, px, b0, v_on, thrL);
            wave_sync();
            // 4. publish the previous macroblock (the row below needs nothing else of this one), then edges 1..3 from
            //    the registers already held
            store_prev(mx, true);
            db_inner_vertical<BS4>(L, px, b0, v_on, thr);
            // the top apron is needed from here on and not before (the vertical edges touch rows 0..15 only): wait until
            // every granule of the macroblock above carries this picture's tag
            // every granule of the macroblock above carries this picture's tag - where the top edge is filtered: only then has the
            // row above handed its bottom rows down (db_hands_down, from the same word), and only then does edge 0 of
            // db_horizontal look at rows -4..-1
            const bool top_on = !first_row && b1.x != 0;
            DB_COUNT(if (top_on) cnt.top_on++;
                     if (!db_any(b0, b1) && !(mx > 0 && (db_hands_down(last_row, prev_tn) || db_dirty(prev_own, true, b0)))) cnt.idle++;)
            if (top_on) {
                db_wait_tags(lane < 24, g, handoff + ((size_t)grow * D.mbw + mx) * 24 + glane, R.serial, timed_out, cnt);
                db_put_apron(s_y, lane, (uint32_t)g);
            }
            wave_sync();
            // 5. horizontal edges
            db_horizontal<BS4>(L, b1, h_on, thrT, thr);
            wave_sync();
            consume();   // the next macroblock's data has arrived; nothing below waits for memory any more
            // 6. the top apron (rows 12..15 / 6..7 of the macroblock above) is final: store it
            if (top_on) db_store_apron(D, s_y, lane, mx, my);
        }
        if (!have_cur) store_prev(mx, false);   // after the last macroblock of the row
        prev_tn = tn; prev_own = db_any(b0, b1);
        cur_y = pf_y; cur_c = pf_c; b0 = pf_b0; b1 = pf_b1; g = pf_g; cur_q = pf_q; tn = pf_tn;
        wave_sync();
    }
    if (timed_out && lane == 0) *R.err = 1u;  // pinned host word, read after the picture's event
    DB_COUNT(db_count_flush(cnt, lane, false);)
}
// The kernels: workgroup (row, y) filters its row of pictures y, y + gridDim.y, ... of the step's R.npic pictures.  A launch whose
// pictures nearly all return at once - the stream hub's bS 4 launch on P steps of content without intra macroblocks - is made with
// gridDim.y = 1: placing a thousand 120-register waves beside the other instance's kernels for nothing is what costs, not the walk
// (see k_pintra_rows).
template <bool BS4, bool PERMB = false, bool IND = false>
__global__ __launch_bounds__(64) void k_deblock_rows(DbRowParams R)
{
    static_assert(!PERMB || IND, "thresholds per edge: the pictures of a decoder group's step");
    __shared__ __attribute__((aligned(16))) uint8_t s_y[DR_TILE];   // (the kernel's, not the picture function's: k_deblock_rows_p inlines two of those)
    // dependency-bound: when a throughput kernel of another stream shares the SIMD, this wave issues first
    __builtin_amdgcn_s_setprio(3);
    for (int pos = blockIdx.y; pos < R.npic; pos += gridDim.y) deblock_rows_picture<BS4, PERMB, IND>(R, pos, (int)threadIdx.x, s_y);
}
// P steps of the encoder's own batches: ONE launch, every picture in the form it needs - with the bS 4 filter when the picture holds intra
// macroblocks (k_pintra_rows' flag), without it otherwise.  The choice is a scalar compare per picture and both bodies are inlined;
// R.need_intra is 0.  (Two launches, one per form, each returning at once from the other's pictures, were a kernel boundary and a
// grid of waves to place on every P step for a launch that on ordinary content finds nothing.)
__device__ __forceinline__ bool db_picture_has_intra(const DbRowParams& R, const int pos)
{
    return R.anyintra[batch_item<false>(R.itemtab, pos)] == R.pic_serial;
}
__global__ __launch_bounds__(64) void k_deblock_rows_p(DbRowParams R)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_y[DR_TILE];
    __builtin_amdgcn_s_setprio(3);
    for (int pos = blockIdx.y; pos < R.npic; pos += gridDim.y) {
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        if (db_picture_has_intra(R, pos)) deblock_rows_picture<true, false, false>(R, pos, lane, s_y);
        else deblock_rows_picture<false, false, false>(R, pos, lane, s_y);
    }
}


// ===========================================================================
// Pair form of the persistent loop filter: ONE wave filters TWO macroblock rows - lanes 0..31 row 2p
// (macroblock t in iteration t), lanes 32..63 row 2p + 1 ONE macroblock behind (macroblock t - 1).  Both rows run the SAME
// instruction stream: every phase of the row form used lanes 0..31 only for the filter arithmetic, so a lockstep batch needs
// half the waves and half the filter instructions per macroblock, and the upper row hands its bottom sample rows to the lower
// one through LDS instead of 24 global granules and their latency.  Inside an iteration the order is the dependency of 8.7
// itself: left edge of V(t) above and of V(t - 1) below; the upper row publishes macroblock t - 1 (final now) into the ring
// slot (t - 1) & 1, the lower row macroblock t - 2 to the next pair; edges 1..3; the lower row takes that slot as its top apron
// (the upper row waits for the previous pair's granules at the same point); horizontal edges of t above and t - 1 below.  A
// slot is written and read in the same iteration, so of the two slots the one not being written is simply idle; the
// upper row's closing publish (t == mbw: no macroblock of its own, no shift) sits at the same point of the iteration, because
// the lower row's last macroblock takes it a few instructions later.  Between pairs the hand-off is
// the row form's ({tag, 4 samples} granules in global memory), and so is everything else: tile layout, the branch-free
// filter, prefetch one macroblock ahead, one writer per picture sample, bounded spins.
// MEASURED (bench workload, 32 pictures per launch): at first the launch got 7 % shorter and the pipeline 1 % slower (each step of
// the critical path carries the data movement of two macroblocks with 32 lanes per row instead of 64, and the waves the row form
// had too many of were asleep in their hand-off spins, not contending for issue).  With the edge skip (an edge no line of
// which is filtered costs one scalar branch) the instruction count decides: 152 VALU per macroblock here, 181 in the row form,
// half the waves - 25.0 k fps against 24.0 k on one box.  So this form is the default from a lockstep batch of 8 pictures on
// (pictures of one slice; MI355X_H264_PAIR_FILTER=N moves the threshold, 0 turns it off); smaller batches, the latency mode and
// the decoder use the row form.  tests/test_gpu_parity.py runs both forms at batch 8 and this one forced on single pictures.
// ===========================================================================
template <bool BS4, bool IND>
__device__ __forceinline__ void deblock_pairs_picture(const DbRowParams& R, const int pos, const int lane, uint8_t (* const s_yy)[DR_PAIR_TILE], uint32_t (* const s_ring)[24])
{
    DbParams D; u64* handoff; const uint32_t* bsw;
    if (!db_picture_view<false, IND>(R, pos, D, handoff, bsw)) return;
    const int half = lane >> 5, hl = lane & 31, cs = D.cw / 2;
    const int rowA = R.row0 + 2 * (int)blockIdx.x, rowB = rowA + 1;
    const bool hasB = rowB < D.mbh;                 // (an odd number of rows: the last wave has an upper row only)
    const int my = half ? (hasB ? rowB : rowA) : rowA;
    const bool live = half == 0 || hasB;            // lanes 32..63 of a wave without a lower row idle along on row A's addresses and store nothing
    const bool first_row = half == 0 && rowA == 0;  // (one slice: only picture row 0 has nothing above)
    const bool last_row = my == D.mbh - 1;
    const bool from_lds = half == 1;                // the lower row's top apron comes from the upper row through LDS
    uint8_t* const s_y = s_yy[half];
    bool timed_out = false;
    // luma dwords owned by this lane: two of the 64 of a macroblock (rows yr0 and yr0 + 8); chroma dword as in the row form
    const int yr0 = hl >> 2, yc4 = (hl & 3) * 4;
    const int cpl_l = (hl >> 4) & 1, cr_l = (hl >> 1) & 7, cc4 = (hl & 1) * 4;
    const DbLane L = db_lane(hl, s_y);
    const DbThr thr = db_picture_thr(D, L.isC);   // one set for every edge of the picture

    uint32_t pf_y0 = 0, pf_y1 = 0, pf_c = 0;
    uint4 pf_b0 = {0, 0, 0, 0}, pf_b1 = pf_b0;
    u64 pf_g = 0;
    uint32_t pf_tn = 0;   // top-edge strengths of the macroblock below this lane's row, as in the row form.  (For the upper row that is
                          // the lower half's b1.x of the same iteration; the load is issued for all 64 lanes either way, so both rows
                          // take the word the same way and no lane is read across.)
    const int trow = last_row ? my : my + 1;
    // only the upper row reads global granules (those of the row above it); a first row and the lanes of the lower row read
    // and ignore row A's own slots - never row -1
    const int grow = (first_row || half == 1) ? rowA : rowA - 1;
    const int glane = hl < 24 ? hl : hl - 24;
    const int last_mx = D.mbw - 1;
    auto prefetch = [&](int mx) {   // mx clamped by the caller into 0 .. mbw - 1
        pf_y0 = *(const uint32_t*)(D.pl[0] + (size_t)(16 * my + yr0) * D.cw + 16 * mx + yc4);
        pf_y1 = *(const uint32_t*)(D.pl[0] + (size_t)(16 * my + yr0 + 8) * D.cw + 16 * mx + yc4);
        pf_c = *(const uint32_t*)((cpl_l ? D.pl[2] : D.pl[1]) + (size_t)(8 * my + cr_l) * cs + 8 * mx + cc4);
        const uint4* b = (const uint4*)(bsw + ((size_t)my * D.mbw + mx) * 8);
        pf_b0 = b[0]; pf_b1 = b[1];
        pf_g = AT_LOAD(handoff + ((size_t)grow * D.mbw + mx) * 24 + glane);
        pf_tn = bsw[((size_t)trow * D.mbw + mx) * 8 + 4];
    };
    auto consume = [&]() {
        asm volatile("" : "+v"(pf_y0), "+v"(pf_y1), "+v"(pf_c), "+v"(pf_g), "+v"(pf_tn));
        asm volatile("" : "+v"(pf_b0.x), "+v"(pf_b0.y), "+v"(pf_b0.z), "+v"(pf_b0.w));
        asm volatile("" : "+v"(pf_b1.x), "+v"(pf_b1.y), "+v"(pf_b1.z), "+v"(pf_b1.w));
    };
    prefetch(0);
    consume();
    uint32_t cur_y0 = pf_y0, cur_y1 = pf_y1, cur_c = pf_c;
    uint4 b0 = pf_b0, b1 = pf_b1;
    u64 g = pf_g;
    uint32_t tn = pf_tn, prev_tn = 0, prev_own = 0;   // prev_*: of macroblock mx - 1, which store_prev serves
    DbCount cnt = DB_COUNT_ZERO;

    // the previous macroblock of this lane's row is final for the row: what the filter can have changed of it goes to the picture,
    // rows 12..15 are handed down where the row below filters its top edge (db_hands_down) - the upper row into the LDS ring, the
    // lower row as global granules for the next pair - and go to the picture with the rest where it does not
    auto store_prev = [&](const int mx, const bool have_cur) {
        if (mx > 0 && live) {
            const int pmx = mx - 1;
            const int co = have_cur ? -16 : 0, cco = have_cur ? -8 : 0;
            const bool down = db_hands_down(last_row, prev_tn), dirty = db_dirty(prev_own, have_cur, b0);
            const int nrow = down ? 12 : 16, ncrow = down ? 6 : 8;
            DB_COUNT(if (!dirty) cnt.skipped++; if (down) cnt.published++;)
            if (dirty) *(uint32_t*)(D.pl[0] + (size_t)(16 * my + yr0) * D.cw + 16 * pmx + yc4) = dw(db_y(s_y, yr0, co + yc4));
            if (dirty && yr0 + 8 < nrow) *(uint32_t*)(D.pl[0] + (size_t)(16 * my + yr0 + 8) * D.cw + 16 * pmx + yc4) = dw(db_y(s_y, yr0 + 8, co + yc4));
            if (dirty && cr_l < ncrow)
                *(uint32_t*)((cpl_l ? D.pl[2] : D.pl[1]) + (size_t)(8 * my + cr_l) * cs + 8 * pmx + cc4) = dw(db_c(s_y, cpl_l, cr_l, cco + cc4));
            if (down && hl < 24) {
                const uint32_t v = db_bottom_dword(s_y, hl, have_cur);
                if (half == 0) s_ring[pmx & 1][hl] = v;
                else AT_STORE(handoff + ((size_t)my * D.mbw + pmx) * 24 + hl, ((u64)R.serial << 32) | v);
            }
        }
    };
    for (int t = 0; t <= D.mbw + 1; t++) {
        const int mx = t - half;                                  // this lane's macroblock
        const bool in_range = mx >= 0 && mx <= D.mbw && live;     // (mx == mbw: the closing store of the row)
        const bool have_cur = in_range && mx < D.mbw;
        if (have_cur) {
            if (mx > 0) {
                dw(db_y(s_y, yr0, yc4 - 16)) = dw(db_y(s_y, yr0, yc4));
                dw(db_y(s_y, yr0 + 8, yc4 - 16)) = dw(db_y(s_y, yr0 + 8, yc4));
                dw(db_c(s_y, cpl_l, cr_l, cc4 - 8)) = dw(db_c(s_y, cpl_l, cr_l, cc4));
            }
        }
        wave_sync();
        if (have_cur) {
            dw(db_y(s_y, yr0, yc4)) = cur_y0;
            dw(db_y(s_y, yr0 + 8, yc4)) = cur_y1;
            dw(db_c(s_y, cpl_l, cr_l, cc4)) = cur_c;
        }
        {   // requests for this lane's next macroblock (clamped: the loads of a finished or not yet started row are harmless)
            const int nx = mx + 1 < 0 ? 0 : (mx + 1 > last_mx ? last_mx : mx + 1);
            prefetch(nx);
        }
        wave_sync();
        const bool v_on = have_cur && (b0.x | b0.y | b0.z | b0.w) != 0, h_on = have_cur && (b1.x | b1.y | b1.z | b1.w) != 0;
        int px[20];
        db_left_edge<BS4>(L, px, b0, v_on, thr);
        wave_sync();
        // the previous macroblock of each row is final now: the upper row's goes into the ring slot the lower row reads further
        // down in this same iteration, the lower row's to the next pair.  mx == mbw is the closing publish of a row (no shift,
        // no left edge) - at this point too, because the lower row's last macroblock is waiting for it.
        if (in_range) store_prev(mx, have_cur);
        db_inner_vertical<BS4>(L, px, b0, v_on, thr);
        wave_sync();   // (the ring slot written above is read by the other half's lanes)
        // top apron, needed by the horizontal edges only: the upper row waits for the previous pair's granules, the lower row
        // takes the ring slot the upper row has just filled
        // - each where its top edge is filtered, which is where the row above has handed anything down
        const bool top_on = have_cur && !first_row && b1.x != 0;
        DB_COUNT(if (top_on) cnt.top_on++;
                 if (__ballot(in_range && ((have_cur && db_any(b0, b1) != 0) || (mx > 0 && (db_hands_down(last_row, prev_tn) || db_dirty(prev_own, have_cur, b0))))) == 0ull) cnt.idle++;)
        db_wait_tags(top_on && !from_lds && hl < 24, g, handoff + ((size_t)grow * D.mbw + mx) * 24 + glane, R.serial, timed_out, cnt);
        if (top_on && hl < 24) db_put_apron(s_y, hl, from_lds ? s_ring[mx & 1][hl] : (uint32_t)g);
        wave_sync();
        db_horizontal<BS4>(L, b1, h_on, thr, thr);
        wave_sync();
        consume();
        // the top apron (rows 12..15 / 6..7 of the macroblock above) is final: store it
        if (top_on && hl < 24) db_store_apron(D, s_y, hl, mx, my);
        if (have_cur) { prev_tn = tn; prev_own = db_any(b0, b1); }
        if (mx + 1 >= 0 && mx + 1 <= last_mx) { cur_y0 = pf_y0; cur_y1 = pf_y1; cur_c = pf_c; b0 = pf_b0; b1 = pf_b1; g = pf_g; tn = pf_tn; }
        wave_sync();
    }
    if (timed_out && lane == 0) *R.err = 1u;
    DB_COUNT(db_count_flush(cnt, lane, true);)
}
template <bool BS4, bool IND = false>
__global__ __launch_bounds__(64) void k_deblock_pairs(DbRowParams R)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_yy[2][DR_PAIR_TILE];   // one tile per row of the pair
    __shared__ __attribute__((aligned(16))) uint32_t s_ring[2][24];   // bottom rows of the upper row's macroblock (parity of its index): 16 luma + 8 chroma dwords
    __builtin_amdgcn_s_setprio(3);
    for (int pos = blockIdx.y; pos < R.npic; pos += gridDim.y) deblock_pairs_picture<BS4, IND>(R, pos, (int)threadIdx.x, s_yy, s_ring);
}
__global__ __launch_bounds__(64) void k_deblock_pairs_p(DbRowParams R)   // P steps: see k_deblock_rows_p
{
    __shared__ __attribute__((aligned(16))) uint8_t s_yy[2][DR_PAIR_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t s_ring[2][24];
    __builtin_amdgcn_s_setprio(3);
    for (int pos = blockIdx.y; pos < R.npic; pos += gridDim.y) {
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        if (db_picture_has_intra(R, pos)) deblock_pairs_picture<true, false>(R, pos, lane, s_yy, s_ring);
        else deblock_pairs_picture<false, false>(R, pos, lane, s_yy, s_ring);
    }
}

}  // namespace h264
