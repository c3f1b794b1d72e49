// media_amd/csrc/host_framing.h -- everything the host writes around the kernels' payload, and the tables it prepares for
// them: parameter sets, slice header, NAL wrapping and emulation prevention, level choice, quantiser / loop-filter
// constants by QP, the picture-sequence state of one stream.  No HIP here: plain values in, bytes and constants out, so a
// host compiler builds (and a sanitizer sees) this file alone.  Part of the one translation unit mi355x_h264.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "item_word.h"   // ItemPic

namespace {

// floor(2^32 / n) + 1: x / n = mulhi(x, inv) for the ranges dev_common.h states (SliceRows, MbDiv); n = 1 has no 32-bit
// reciprocal and is flagged by 0
inline unsigned recip32(int n) { return n > 1 ? (unsigned)(0x100000000ull / (unsigned)n) + 1u : 0u; }

// the one error text of an engine, a stream or a decoder: formats into its char[256] and hands the code back
template <size_t N>
int set_err(char (&err)[N], int code, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(err, N, fmt, ap); va_end(ap);
    return code;
}

// Where a stream stands in its picture sequence: the engine keeps one (its batch items move in lockstep), the stream hub
// one per stream.
// Temporal layers (include/mi355x_h264.h, "temporal layers"): with layers = 2 the pictures at odd positions of a GOP are layer 1 -
// P pictures nobody refers to.  frame_in_gop is the POSITION in the GOP (every picture counts: next_is_idr, layer); refs_in_gop
// counts the reference pictures since the IDR picture (avail_refs).  After a layer-1 picture cur, frame_num and refs_in_gop are what
// the layer-0 picture before it left: it is reconstructed into the ring slot the next layer-0 picture overwrites and carries that
// picture's frame_num (PrevRefFrameNum + 1, 7.4.3).  layers = 1: the two counts move together and every picture is layer 0.
// Intra refresh (include/mi355x_h264.h, "intra refresh"): refresh_n = n bands (0: off), and p, the count of P pictures since the
// last IDR picture, is the position frame_in_gop of the picture begun - refresh needs one layer, so every picture counts, and
// whatever makes an IDR picture (gop, force_idr, a scene change, a failed picture) restarts it with begin().
struct PicSeq {
    int cur = 0;                 // ring slot the next picture is reconstructed into
    int frame_in_gop = 0, frame_num = 0, idr_id = 0, force_idr = 0;
    long frames = 0;
    int layers = 1, refs_in_gop = 0;
    int last_cur = -1;           // ring slot of the last picture that went out (-1: none yet)
    bool next_is_idr(int gop) const { return force_idr || frames == 0 || frame_in_gop >= gop; }
    void begin(bool idr) { if (idr) { frame_in_gop = 0; refs_in_gop = 0; frame_num = 0; force_idr = 0; } }
    // of the picture begun: its layer, and the two facts k_me takes (item_word.h ME_PARK, ME_SEED_PARK)
    int layer() const { return layers == 2 ? (frame_in_gop & 1) : 0; }
    int me_facts(bool idr) const { return layers != 2 || idr ? 0 : layer() ? 1 : 2; }
    int refresh_n = 0;           // intra refresh: the number of bands (the stream's slices), 0 = off
    int refresh_p() const { return frame_in_gop; }   // of the picture begun: 1, 2, .. for the P pictures since the IDR picture
    // the band of the picture begun that is coded all intra: k = (p - 1) mod n; -1 for an IDR picture or with refresh off
    int refresh_band(bool idr) const { return refresh_n < 2 || idr || refresh_p() < 1 ? -1 : (refresh_p() - 1) % refresh_n; }
    // reference pictures the picture begun has, of a stream that searches nrefs: those coded since the stream's last IDR picture
    // (0, 1, 2, .. up to nrefs).  The one rule of the engine and the stream hub: a forced IDR restarts it with begin()
    int avail_refs(bool idr, int nrefs) const { return idr ? 0 : std::min(nrefs, refs_in_gop); }
    // the record of the picture begun (engine.h, Step): batch item `item` of a stream that codes at qp and searches nrefs pictures
    ItemPic pic(int item, int qp, bool idr, int nrefs) const
    {
        return ItemPic{item, cur, qp, frame_num, idr_id, avail_refs(idr, nrefs), layer(), me_facts(idr), refresh_band(idr)};
    }
    // the slot of the last picture that went out (before the first: the slot behind cur, as ever)
    int last_slot(int nbuf) const { return last_cur >= 0 ? last_cur : (cur + nbuf - 1) % nbuf; }
    // the picture went out: idr_step = what an IDR picture adds to idr_pic_id (the engine: its stride times the batch)
    void advance(bool idr, int nbuf, int idr_step)
    {
        last_cur = cur;
        if (!layer()) { cur = (cur + 1) % nbuf; frame_num = (frame_num + 1) & 255; refs_in_gop++; }
        frame_in_gop++; frames++;
        if (idr) idr_id = (idr_id + idr_step) & 0xFF;
    }
};
// Intra refresh wants n = 2 .. 32 bands and the picture to have exactly that many: the bands the engine makes of `slices` for a
// picture of mbh macroblock rows (create_engine's rule: ceil(mbh / slices) rows each, at least two), 0 for a count out of range
inline int refresh_bands(int mbh, int slices)
{
    if (slices < 2 || slices > 32) return 0;
    const int n = std::min(slices, std::max(1, mbh / 2)), rows = (mbh + n - 1) / n;
    return (mbh + rows - 1) / rows;
}
// the record of item g of a direct batch, from item 0's: the items move in lockstep and differ in their idr_pic_id alone, which
// steps by the engine's stride (mi355x_h264_set_idr_pic_id) and wraps at 256
inline ItemPic batch_item_pic(ItemPic p, int g, int idr_step) { p.item = g; p.idr_id = (p.idr_id + g * idr_step) & 0xFF; return p; }
// first byte of a slice NAL unit: nal_ref_idc 3 for an IDR picture, 2 for a P picture others refer to, 0 for a layer-1 picture
inline int slice_nal_hdr(bool idr, int layer) { return idr ? ((3 << 5) | 5) : layer ? 1 : ((2 << 5) | 1); }

// ---- host tables (ITU-T H.264 Table 8-15, A-1; quantiser of the reference model) ----
const uint8_t h_chroma_qp[52] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                                 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33,
                                 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};
const uint8_t h_dequant_v[6][3] = {{10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};
const uint16_t h_quant_mf[6][3] = {{13107, 5243, 8066}, {11916, 4660, 7490}, {10082, 4194, 6554},
                                   {9362, 3647, 5825},  {8192, 3355, 5243},  {7282, 2893, 4559}};
const uint8_t h_lambda[52] = {1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  1,  2,  2,
                              2,  2,  3,  3,  3,  4,  4,  4,  5,  6,  6,  7,  8,  9,  10, 11, 13, 14,
                              16, 18, 20, 23, 25, 29, 32, 36, 40, 45, 51, 57, 64, 72, 81, 91};
const struct { uint8_t idc; uint32_t mbps, fs; } h_levels[] = {
    {10, 1485, 99},     {11, 3000, 396},     {12, 6000, 396},     {13, 11880, 396},   {20, 11880, 396},  {21, 19800, 792},
    {22, 20250, 1620},  {30, 40500, 1620},   {31, 108000, 3600},  {32, 216000, 5120}, {40, 245760, 8192}, {41, 245760, 8192},
    {42, 522240, 8704}, {50, 589824, 22080}, {51, 983040, 36864}, {52, 2073600, 36864}};
const uint8_t h_alpha[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,   0,   0,   0,   4,   4,
                             5,  6,  7,  8,  9,  10, 12, 13, 15, 17, 20, 22, 25,  28,  32,  36,  40,  45,
                             50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203, 226, 255, 255};
const uint8_t h_beta[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  2,  2,
                            2,  3,  3,  3,  3,  4,  4,  4,  6,  6,  7,  7,  8,  8,  9,  9,  10, 10,
                            11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18};
const uint8_t h_tc0[52][3] = {
    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},    {0, 0, 0},    {0, 0, 0},    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},  {0, 0, 0},
    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},    {0, 0, 0},    {0, 0, 0},    {0, 0, 0},   {0, 0, 0},   {0, 0, 0},  {0, 0, 1},
    {0, 0, 1},   {0, 0, 1},   {0, 0, 1},    {0, 1, 1},    {0, 1, 1},    {1, 1, 1},   {1, 1, 1},   {1, 1, 1},  {1, 1, 1},
    {1, 1, 2},   {1, 1, 2},   {1, 1, 2},    {1, 1, 2},    {1, 2, 3},    {1, 2, 3},   {2, 2, 3},   {2, 2, 4},  {2, 3, 4},
    {2, 3, 4},   {3, 3, 5},   {3, 4, 6},    {3, 4, 6},    {4, 5, 7},    {4, 5, 8},   {4, 6, 9},   {5, 7, 10}, {6, 8, 11},
    {6, 8, 13},  {7, 10, 14}, {8, 11, 16},  {9, 12, 18},  {10, 13, 20}, {11, 15, 23}, {13, 17, 25}};

// ---- host bit writer for parameter sets and slice headers ----
struct HostBits {
    std::vector<uint8_t> bytes;
    uint64_t nbits = 0;
    void put(int n, uint32_t v)
    {
        for (int i = n - 1; i >= 0; i--) {
            if ((nbits >> 3) >= bytes.size()) bytes.push_back(0);
            if ((v >> i) & 1) bytes[nbits >> 3] |= (uint8_t)(0x80 >> (nbits & 7));
            nbits++;
        }
    }
    void ue(uint32_t v)
    {
        uint32_t x = v + 1;
        int n = 0;
        while ((x >> n) > 1) n++;
        put(n, 0);
        put(n + 1, x);
    }
    void se(int32_t v) { ue(v > 0 ? (uint32_t)(2 * v - 1) : (uint32_t)(-2 * v)); }
    void trailing()
    {
        put(1, 1);
        while (nbits & 7) put(1, 0);
    }
};

size_t nal_escape(const uint8_t* rbsp, size_t n, uint8_t* out)
{
    size_t o = 0;
    int zeros = 0;
    for (size_t i = 0; i < n; i++) {
        if (zeros == 2 && rbsp[i] <= 3) { out[o++] = 3; zeros = 0; }
        out[o++] = rbsp[i];
        zeros = rbsp[i] == 0 ? zeros + 1 : 0;
    }
    return o;
}

void append_nal(std::vector<uint8_t>& au, int ref_idc, int type, const HostBits& b)
{
    const uint8_t sc[5] = {0, 0, 0, 1, (uint8_t)((ref_idc << 5) | type)};
    au.insert(au.end(), sc, sc + 5);
    std::vector<uint8_t> esc(b.bytes.size() * 3 / 2 + 4);
    const size_t n = nal_escape(b.bytes.data(), b.bytes.size(), esc.data());
    au.insert(au.end(), esc.begin(), esc.begin() + n);
}

// Recovery point SEI (D.1.7 / D.2.7) in front of the access unit that starts a refresh cycle (band 0 all intra): NAL type 6,
// nal_ref_idc 0, one message of payload type 6 - recovery_frame_cnt = n - 1 (after the n pictures of the cycle every band has been
// coded intra once and predicted from refreshed rows only), exact_match_flag 1, broken_link_flag 0, changing_slice_group_idc 0.
// Appended to `au` with its start code, through nal_escape like every NAL unit.
inline void append_recovery_point_sei(std::vector<uint8_t>& au, int n)
{
    HostBits pl;
    pl.ue((uint32_t)n - 1); pl.put(1, 1); pl.put(1, 0); pl.put(2, 0);
    if (pl.nbits & 7) pl.trailing();   // sei_payload(): bit_equal_to_one, then zero bits up to the byte boundary
    HostBits b;
    b.put(8, 6);                            // payloadType
    b.put(8, (uint32_t)pl.bytes.size());    // payloadSize
    for (uint8_t v : pl.bytes) b.put(8, v);
    b.trailing();
    append_nal(au, 0, 6, b);
}

template <class Quant>
void fill_quant(Quant& q, int qp)
{
    q.qp = qp;
    q.qbits = 15 + qp / 6;
    q.f_intra = (1 << q.qbits) / 3;
    q.f_inter = (1 << q.qbits) / 6;
    for (int c = 0; c < 3; c++) {
        q.mf[c] = h_quant_mf[qp % 6][c];
        q.dq[c] = h_dequant_v[qp % 6][c] << (qp / 6);
        q.thr_inter[c] = (int)((((int64_t)1 << q.qbits) - q.f_inter + q.mf[c] - 1) / q.mf[c]);
    }
    q.thr_dc_inter = (int)((((int64_t)1 << (q.qbits + 1)) - 2 * (int64_t)q.f_inter + q.mf[0] - 1) / q.mf[0]);
    static const uint8_t v8[6][6] = {{20, 18, 32, 19, 25, 24}, {22, 19, 35, 21, 28, 26}, {26, 23, 42, 24, 33, 31},
                                     {28, 25, 45, 26, 35, 33}, {32, 28, 51, 30, 40, 38}, {36, 32, 58, 34, 46, 43}};
    static const uint16_t m8[6][6] = {{13107, 11428, 20972, 12222, 16777, 15481}, {11916, 10826, 19174, 11058, 14980, 14290},
                                      {10082, 8943, 15978, 9675, 12710, 11985},   {9362, 8228, 14913, 8931, 11984, 11259},
                                      {8192, 7346, 13159, 7740, 10486, 9777},     {7282, 6428, 11570, 6830, 9118, 8640}};
    for (int c = 0; c < 6; c++) { q.mf8[c] = m8[qp % 6][c]; q.ls8[c] = 16 * v8[qp % 6][c]; }
}

// everything one picture QP fixes for the kernels (FrameParams qy / qc / lambda / sad_nz; QpEntry of the indirect launches)
template <class Quant>
void fill_qp(Quant& qy, Quant& qc, int& lambda, int& sad_nz, int qp)
{
    fill_quant(qy, qp);
    fill_quant(qc, h_chroma_qp[qp]);
    lambda = h_lambda[qp];
    // k_me's shortcut for the "quantises to nothing" test: 64 sqrt(sum over the 16 positions of t^2 / (n_i n_j)), rounded up
    const double t0 = qy.thr_inter[0], t1 = qy.thr_inter[1], t2 = qy.thr_inter[2];
    sad_nz = (int)std::ceil(64.0 * std::sqrt(4 * t0 * t0 / 16.0 + 4 * t1 * t1 / 100.0 + 8 * t2 * t2 / 40.0)) + 1;
}
// alpha / beta / tc0 of 8.7.2.2 for a picture of one QP (D: DbParams of k_deblock.h)
template <class Db>
void fill_filter_thresholds(Db& D, int qp)
{
    const int qpc = h_chroma_qp[qp];
    D.alpha_y = h_alpha[qp]; D.beta_y = h_beta[qp]; D.alpha_c = h_alpha[qpc]; D.beta_c = h_beta[qpc];
    for (int i = 0; i < 3; i++) { D.tc0_y[i] = h_tc0[qp][i]; D.tc0_c[i] = h_tc0[qpc][i]; }
}

// what the parameter sets and slice headers of a stream depend on
// described: the stream carries a colour description (include/mi355x_h264.h, "colour description") and its SPS ends with a VUI;
// matrix (1 BT.709, 6 BT.601), full_range, chroma_loc (streams of RGBA input: chroma_loc_info is written) and fps are its contents.
// 0 (every undescribed stream): the SPS is what it was before there were descriptions
// refresh: intra refresh is on (nsl bands).  No byte of the parameter sets or slice headers depends on it; it is here because the
// engine of such a stream launches another form of k_me, so it shares no engine with an ordinary stream of nsl slices (hub.h)
struct StreamShape { int profile_idc, level_idc, nrefs, mbw, mbh, width, height, nsl, disable_deblock, described, matrix, full_range, chroma_loc, fps, refresh; };

// A colour description as its owner keeps it, and the variant of the two conversions it selects: 0 BT.601 limited (what an
// undescribed stream has), 1 BT.709 limited, 2 BT.601 full, 3 BT.709 full
struct ColourDesc { int described = 0, matrix = 6, full_range = 0; };
inline bool colour_valid(int matrix, int full_range) { return (matrix == 1 || matrix == 6) && (full_range == 0 || full_range == 1); }
inline int colour_variant(int matrix, int full_range) { return (matrix == 1 ? 1 : 0) | (full_range ? 2 : 0); }
inline bool same_colour(const ColourDesc& a, const ColourDesc& b)
{
    return a.described == b.described && (!a.described || (a.matrix == b.matrix && a.full_range == b.full_range));
}

// vui_parameters() of E.1.1 for a described stream, behind vui_parameters_present_flag = 1
inline void write_vui(HostBits& s, const StreamShape& f)
{
    s.put(1, 0);  // aspect_ratio_info_present_flag
    s.put(1, 0);  // overscan_info_present_flag
    s.put(1, 1);  // video_signal_type_present_flag
    s.put(3, 5);  // video_format: unspecified
    s.put(1, (uint32_t)f.full_range);
    s.put(1, 1);  // colour_description_present_flag
    const uint32_t prim = f.matrix == 1 ? 1 : 6;   // BT.709: 1 / 1 / 1; BT.601: 6 / 6 / 6
    s.put(8, prim); s.put(8, prim); s.put(8, (uint32_t)f.matrix);
    s.put(1, f.chroma_loc ? 1 : 0);   // chroma_loc_info_present_flag: the 2x2 mean of the RGBA ingest makes centre-sited chroma
    if (f.chroma_loc) { s.ue(1); s.ue(1); }
    s.put(1, 1);  // timing_info_present_flag
    s.put(32, 1); s.put(32, 2u * (uint32_t)f.fps);   // num_units_in_tick, time_scale (a tick is a field)
    s.put(1, 1);  // fixed_frame_rate_flag
    s.put(1, 0); s.put(1, 0);   // nal / vcl_hrd_parameters_present_flag
    s.put(1, 0);  // pic_struct_present_flag
    s.put(1, 1);  // bitstream_restriction_flag
    s.put(1, 1);  // motion_vectors_over_pic_boundaries_flag
    s.ue(0); s.ue(0);     // max_bytes_per_pic_denom, max_bits_per_mb_denom
    s.ue(16); s.ue(16);   // log2_max_mv_length_horizontal / _vertical
    s.ue(0);      // max_num_reorder_frames: output order is decoding order, a decoder may hand out every picture at once
    s.ue((uint32_t)f.nrefs);   // max_dec_frame_buffering
}

// Annex-B SPS + PPS NAL units
std::vector<uint8_t> build_parameter_sets(const StreamShape& f)
{
    const int prof = f.profile_idc;
    HostBits s;
    s.put(8, (uint32_t)prof);
    s.put(8, prof == 66 ? 0xC0 : prof == 77 ? 0x40 : 0x00);
    s.put(8, (uint32_t)f.level_idc);
    s.ue(0);
    if (prof == 100) { s.ue(1); s.ue(0); s.ue(0); s.put(1, 0); s.put(1, 0); }
    s.ue(4);      // log2_max_frame_num_minus4
    s.ue(2);      // pic_order_cnt_type
    s.ue((uint32_t)f.nrefs);   // max_num_ref_frames (ref :290: 1; config.refs)
    s.put(1, 0);  // gaps_in_frame_num_value_allowed_flag
    s.ue((uint32_t)f.mbw - 1);
    s.ue((uint32_t)f.mbh - 1);
    s.put(1, 1);  // frame_mbs_only_flag
    s.put(1, 1);  // direct_8x8_inference_flag
    const int cr = (f.mbw * 16 - f.width) / 2, cb = (f.mbh * 16 - f.height) / 2;
    if (cr || cb) { s.put(1, 1); s.ue(0); s.ue((uint32_t)cr); s.ue(0); s.ue((uint32_t)cb); }
    else s.put(1, 0);
    if (f.described) { s.put(1, 1); write_vui(s, f); }
    else s.put(1, 0);  // vui_parameters_present_flag
    s.trailing();
    HostBits p;
    p.ue(0); p.ue(0);
    p.put(1, 0);  // CAVLC
    p.put(1, 0);
    p.ue(0); p.ue((uint32_t)f.nrefs - 1); p.ue(0);   // slice groups, num_ref_idx_l0 / l1_default_active_minus1
    p.put(1, 0); p.put(2, 0);
    p.se(0); p.se(0); p.se(0);
    p.put(1, 1);  // deblocking_filter_control_present_flag
    p.put(1, 0); p.put(1, 0);
    if (prof == 100) { p.put(1, 1); p.put(1, 0); p.se(0); }   // transform_8x8_mode_flag = 1: inter macroblocks use the 8x8 transform (k_tq8)
    p.trailing();
    std::vector<uint8_t> out;
    append_nal(out, 3, 7, s);
    append_nal(out, 3, 8, p);
    return out;
}

// slice_header() of 7.3.3 for this build's fixed choices, from slice_type on (first_mb_in_slice differs per slice and
// is written by k_bit_scan); returns bit count (< 64).
// frame_num, qp, nact (num_ref_idx_l0_active of a P slice): the picture's own - one per batch item in the stream hub's steps
// nonref: a layer-1 picture (nal_ref_idc 0) - its header has no dec_ref_pic_marking()
int build_slice_header(const StreamShape& f, bool idr, int idr_id, bool no_filter, int frame_num, int qp, int nact, uint64_t* bits, bool nonref = false)
{
    HostBits h;
    h.ue(idr ? 7 : 5);
    h.ue(0);
    h.put(8, (uint32_t)frame_num);
    if (idr) h.ue((uint32_t)idr_id);
    if (!idr) {   // num_ref_idx_active_override_flag: the first pictures after an IDR have fewer reference pictures than the PPS announces
        if (nact != f.nrefs) { h.put(1, 1); h.ue((uint32_t)nact - 1); } else h.put(1, 0);
        h.put(1, 0);   // ref_pic_list_modification_flag_l0
    }
    if (idr) { h.put(1, 0); h.put(1, 0); } else if (!nonref) h.put(1, 0);   // dec_ref_pic_marking(): nal_ref_idc != 0 only
    h.se(qp - 26);
    no_filter = no_filter || f.disable_deblock;            // (a picture with an I_PCM macroblock is not filtered)
    h.ue(no_filter ? 1 : f.nsl > 1 ? 2 : 0);   // several slices: no filtering across slice edges, the bands stay independent
    if (!no_filter) { h.se(0); h.se(0); }
    uint64_t v = 0;
    for (uint64_t i = 0; i < h.nbits; i++) v = (v << 1) | ((h.bytes[i >> 3] >> (7 - (i & 7))) & 1);
    *bits = v;
    return (int)h.nbits;
}

// Tight copy of a strided picture: I420 (three planes), NV12 (two) or RGBA (one), for the transfer to the device.  One
// memcpy when the caller's picture is tight already.
enum { PIC_I420 = 0, PIC_NV12 = 1, PIC_RGBA = 2 };
struct HostPicture { int layout; const uint8_t* p[3]; int stride[3]; };
inline size_t picture_bytes(int layout, int w, int h) { return layout == PIC_RGBA ? (size_t)w * h * 4 : (size_t)w * h * 3 / 2; }
inline bool picture_is_tight(const HostPicture& in, int w, int h)
{
    const size_t ysz = (size_t)w * h;
    if (in.layout == PIC_RGBA) return (size_t)in.stride[0] == (size_t)w * 4;
    if (in.layout == PIC_NV12) return in.stride[0] == w && in.stride[1] == w && in.p[1] == in.p[0] + ysz;
    return in.stride[0] == w && in.stride[1] == w / 2 && in.stride[2] == w / 2 && in.p[1] == in.p[0] + ysz && in.p[2] == in.p[1] + ysz / 4;
}
inline void pack_picture(const HostPicture& in, int w, int h, uint8_t* dst)
{
    const int nplanes = in.layout == PIC_RGBA ? 1 : in.layout == PIC_NV12 ? 2 : 3;
    for (int p = 0; p < nplanes; p++) {
        const size_t row = in.layout == PIC_RGBA ? (size_t)w * 4 : (p && in.layout == PIC_I420) ? (size_t)(w / 2) : (size_t)w;
        const int rows = p ? h / 2 : h;
        for (int r = 0; r < rows; r++) memcpy(dst + (size_t)r * row, in.p[p] + (size_t)r * in.stride[p], row);
        dst += row * rows;
    }
}

// Quality report: the metrics the switch takes (include/mi355x_h264.h: bit 0 SSE, bit 1 SSIM).  Off, the SSE alone, or both: the
// SSIM record accompanies the SSE record, so SSIM alone is refused like any other bit.  And what MI355X_H264_QUALITY in the
// environment turns on when an engine is created: "1" the SSE, "3" both, anything else nothing.
bool quality_metrics_ok(unsigned metrics) { return metrics == 0 || metrics == 1 || metrics == 3; }
unsigned quality_env_metrics(const char* v) { return v && (v[0] == '1' || v[0] == '3') && !v[1] ? (unsigned)(v[0] - '0') : 0u; }

int pick_level(int mbs, int fps)
{
    for (const auto& l : h_levels)
        if ((uint32_t)mbs <= l.fs && (uint32_t)(mbs * fps) <= l.mbps) return l.idc;
    return 52;
}

}  // namespace
