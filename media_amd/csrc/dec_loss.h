// media_amd/csrc/dec_loss.h -- the arithmetic of the decoder's conceal mode (include/mi355x_h264_dec.h, "loss mode") that knows
// nothing of HIP and nothing of the parser's classes: where the holes of a picture lie, how many reference pictures a frame_num
// gap stands for and which held picture an entry of the reference list then means, the list of ring slots a concealing stream
// keeps in place of the ring's plain rotation, and the damage map (a byte per macroblock: which samples may differ from the
// lossless decode).  Plain C++ over plain arrays, so that tools/dec_loss_harness.cpp runs it on hand-made pictures with known
// answers under AddressSanitizer (tests/test_dec_loss_host.py), as hub_sched.h and dec_group_sched.h are run.  The parser
// (h264_parse.h) and the decoder groups (dec_group.h) call it; neither repeats it.
#pragma once
#include <stdint.h>
#include <stddef.h>

namespace dec_loss {

enum { TAINTED = 1, CONCEALED = 2 };   // the bits of a damage-map byte
enum { MAX_REFS = 3 };                 // reference pictures a stream holds (the ring has one slot more)
enum { MB_I16 = 0, MB_P16 = 1, MB_PSKIP = 2, MB_IPCM = 3, MB_I4 = 4 };   // = dev_common.h MB_*; every other value: an inter macroblock

// ---- holes: macroblocks no received slice covers.  `expected` is the address behind the last received slice (0 at the start of
// the picture), `next_first` the first_mb_in_slice of the next received slice, or `nmb` at the end of the picture.  The hole is
// [from, to); from == to: there is none
struct Hole { int from, to; };
inline Hole hole_before(int expected, int next_first, int nmb)
{
    const int to = next_first < nmb ? next_first : nmb;
    return Hole{expected, to > expected ? to : expected};
}

// ---- frame_num gaps (7.4.3, 8.2.5.2): reference pictures missing between the previous reference picture and this picture.
// prev_ref_frame_num < 0: no reference picture is held, nothing can be missing
inline int frame_num_gap(int frame_num, int prev_ref_frame_num, int log2_max_frame_num)
{
    if (prev_ref_frame_num < 0) return 0;
    return (frame_num - prev_ref_frame_num - 1) & ((1 << log2_max_frame_num) - 1);
}
// every missing picture stands for a copy of the newest held picture: the entry of age a (0 = the reference picture "decoded" last,
// the stand-ins counted) of the picture behind a gap of g means the held picture of this real age
inline int real_age(int a, int g) { return a > g ? a - g : 0; }
inline int refs_after_gap(int have_refs, int g, int max_refs) { return have_refs + g < max_refs ? have_refs + g : max_refs; }

// ---- the reference pictures of a concealing stream, newest first, as ring slots.  A stream without loss needs no list: its ring
// rotates, and the picture of age a lies in slot cur - 1 - a.  Stand-in pictures are not stored (no step is run for them): they
// share the slot of the picture they copy, and `standin` says that their samples count as tainted whatever that slot's map says
struct RefSlots {
    int slot[MAX_REFS] = {0, 0, 0};
    uint8_t standin[MAX_REFS] = {0, 0, 0};
    // the list a rotating ring stands for: `cur` is written next, `have` pictures are held, `nbuf` slots
    void from_ring(int cur, int have, int nbuf)
    {
        for (int a = 0; a < MAX_REFS; a++) {
            const int age = a < have ? a : (have > 0 ? have - 1 : 0);
            slot[a] = (cur + nbuf - 1 - age) % nbuf;
            standin[a] = 0;
        }
    }
    void push(int s, bool is_standin)
    {
        for (int a = MAX_REFS - 1; a > 0; a--) { slot[a] = slot[a - 1]; standin[a] = standin[a - 1]; }
        slot[0] = s; standin[0] = is_standin ? 1 : 0;
    }
    // g missing reference pictures: g copies of the newest held picture enter the list
    void gap(int g)
    {
        const int newest = slot[0];
        for (int k = 0; k < g && k < MAX_REFS; k++) push(newest, true);
    }
    // a join: every entry is the grey picture in ring slot `grey`
    void join(int grey)
    {
        for (int a = 0; a < MAX_REFS; a++) { slot[a] = grey; standin[a] = 1; }
    }
    // the slot the next picture is written to: the first behind `cur` that none of the `have` held pictures lies in
    int next_free(int cur, int have, int nbuf) const
    {
        for (int d = 1; d <= nbuf; d++) {
            const int s = (cur + d) % nbuf;
            bool used = false;
            for (int a = 0; a < have && a < MAX_REFS; a++) used = used || slot[a] == s;
            if (!used) return s;
        }
        return (cur + 1) % nbuf;
    }
};

// ---- the damage map of one picture.  The rules (conservative, at macroblock granularity):
//   a concealed macroblock is tainted;  I_PCM is clean;
//   an intra macroblock is tainted if a neighbour its prediction may read (A, B, C, D: bits 4..7 of `avail`, which hold "in the
//     same slice, decoded before, and usable under constrained_intra_pred") is tainted;
//   an inter 4x4 block taints its macroblock if a tainted macroblock of the referenced picture overlaps the rectangle it reads:
//     the block, widened by the six-tap margins (2 before, 3 behind) in each direction whose vector component is fractional
//     (8.4.2.2.1), and the 2x2 chroma block, widened by one sample where the component has a fraction of eighths (8.4.2.2.2),
//     every coordinate clamped to the coded picture;  a stand-in picture (ref[r] == nullptr) is tainted everywhere;
//   then, in decoding order, every filtered left and top macroblock edge taints both its macroblocks if either is tainted (the
//     filter reads three samples and may change three on each side, and a changed sample reaches the next edge): an edge is
//     filtered with disable_deblocking_filter_idc 0 when the neighbour lies in the picture, with 2 when it lies in the same slice
//     (bits 0 / 1 of `avail`), never with 1.
struct TaintPic {
    int mbw = 0, mbh = 0;
    const uint8_t* type = nullptr;       // macroblock type of macroblock i at type[i * type_stride]
    size_t type_stride = 1;
    const int16_t* mv4 = nullptr;        // 32 per macroblock: (x, y) of the sixteen 4x4 blocks, raster order, quarter samples
    const uint8_t* refq = nullptr;       // 4 per macroblock: ref_idx_l0 of the 8x8 quadrants
    const uint8_t* avail = nullptr;      // 1 per macroblock (h264_parse.h, Picture::mbavail)
    const uint8_t* concealed = nullptr;  // 1 per macroblock, non-zero: filled in for a hole; nullptr: none
    int deblock_idc = 0;
    const uint8_t* ref[MAX_REFS] = {nullptr, nullptr, nullptr};   // the damage map of RefPicList0 entry r; nullptr: a stand-in
};

inline bool rect_tainted(const uint8_t* map, int mbw, int x0, int x1, int y0, int y1, int maxx, int maxy, int shift)
{
    x0 = x0 < 0 ? 0 : (x0 > maxx ? maxx : x0); x1 = x1 < 0 ? 0 : (x1 > maxx ? maxx : x1);
    y0 = y0 < 0 ? 0 : (y0 > maxy ? maxy : y0); y1 = y1 < 0 ? 0 : (y1 > maxy ? maxy : y1);
    for (int my = y0 >> shift; my <= y1 >> shift; my++)
        for (int mx = x0 >> shift; mx <= x1 >> shift; mx++)
            if (map[(size_t)my * mbw + mx] & TAINTED) return true;
    return false;
}

// out[mbw * mbh] receives the map (out may not alias a ref[] map); returns the tainted macroblocks, *concealed_count those filled in
inline int taint_picture(const TaintPic& p, uint8_t* out, int* concealed_count)
{
    const int W = p.mbw, H = p.mbh, cw = 16 * W, ch = 16 * H;
    int nconc = 0;
    for (int my = 0; my < H; my++)
        for (int mx = 0; mx < W; mx++) {
            const size_t i = (size_t)my * W + mx;
            const int t = p.type[i * p.type_stride];
            uint8_t v = 0;
            if (p.concealed && p.concealed[i]) { v = TAINTED | CONCEALED; nconc++; }
            else if (t == MB_IPCM) v = 0;
            else if (t == MB_I16 || t == MB_I4) {
                const int a = p.avail[i];
                if (((a & 16) && (out[i - 1] & TAINTED)) || ((a & 32) && (out[i - W] & TAINTED)) || ((a & 64) && (out[i - W + 1] & TAINTED)) ||
                    ((a & 128) && (out[i - W - 1] & TAINTED)))
                    v = TAINTED;
            } else {
                for (int b = 0; b < 16 && !v; b++) {
                    const int bx = b & 3, by = b >> 2;
                    int r = p.refq[i * 4 + 2 * (by >> 1) + (bx >> 1)];
                    if (r >= MAX_REFS) r = MAX_REFS - 1;
                    const uint8_t* map = p.ref[r];
                    if (!map) { v = TAINTED; break; }
                    const int vx = p.mv4[i * 32 + 2 * b], vy = p.mv4[i * 32 + 2 * b + 1];
                    const int x = 16 * mx + 4 * bx + (vx >> 2), y = 16 * my + 4 * by + (vy >> 2);
                    const int fx = vx & 3, fy = vy & 3;
                    if (rect_tainted(map, W, x - (fx ? 2 : 0), x + 3 + (fx ? 3 : 0), y - (fy ? 2 : 0), y + 3 + (fy ? 3 : 0), cw - 1, ch - 1, 4)) { v = TAINTED; break; }
                    const int cx = 8 * mx + 2 * bx + (vx >> 3), cy = 8 * my + 2 * by + (vy >> 3);
                    if (rect_tainted(map, W, cx, cx + 1 + ((vx & 7) ? 1 : 0), cy, cy + 1 + ((vy & 7) ? 1 : 0), cw / 2 - 1, ch / 2 - 1, 3)) v = TAINTED;
                }
            }
            out[i] = v;
        }
    if (p.deblock_idc != 1)
        for (int my = 0; my < H; my++)
            for (int mx = 0; mx < W; mx++) {
                const size_t i = (size_t)my * W + mx;
                const int a = p.avail[i];
                const bool left = mx > 0 && (p.deblock_idc == 0 || (a & 1)), top = my > 0 && (p.deblock_idc == 0 || (a & 2));
                if (left && ((out[i] | out[i - 1]) & TAINTED)) { out[i] |= TAINTED; out[i - 1] |= TAINTED; }
                if (top && ((out[i] | out[i - W]) & TAINTED)) { out[i] |= TAINTED; out[i - W] |= TAINTED; }
            }
    int n = 0;
    for (size_t i = 0; i < (size_t)W * H; i++) n += out[i] & TAINTED;
    if (concealed_count) *concealed_count = nconc;
    return n;
}

}  // namespace dec_loss
