// media_amd/csrc/h264_vlc_packed.h -- the CAVLC tables of h264_vlc_tables.h as ONE array of 16-bit entries, code length in
// bits 0..7 and code bits from bit 8 on: the device entropy coder (k_cavlc.h) gets a code with one access instead of two.
// Generated at compile time from the same initialisers; the static_assert below compares every entry with the separate
// length and bits arrays.
#pragma once
#include <stdint.h>
#include "h264_vlc_tables.h"

namespace h264 {

// first entry of every table in VlcPacked::e (the index conventions inside a table are those of h264_vlc_tables.h)
enum { VLC_CT = 0, VLC_CDC = VLC_CT + 4 * 68, VLC_TZ = VLC_CDC + 20, VLC_CTZ = VLC_TZ + 15 * 16, VLC_RUN = VLC_CTZ + 3 * 4, VLC_ENTRIES = VLC_RUN + 7 * 16 };
struct VlcPacked { uint16_t e[VLC_ENTRIES]; };
static_assert(sizeof(VlcPacked) == 1312, "packed CAVLC tables");

namespace vlc_src {
constexpr uint8_t ct_len[4][68] = H264_TAB_CT_LEN, ct_bits[4][68] = H264_TAB_CT_BITS;
constexpr uint8_t cdc_len[20] = H264_TAB_CDC_LEN, cdc_bits[20] = H264_TAB_CDC_BITS;
constexpr uint8_t tz_len[15][16] = H264_TAB_TZ_LEN, tz_bits[15][16] = H264_TAB_TZ_BITS;
constexpr uint8_t ctz_len[3][4] = H264_TAB_CTZ_LEN, ctz_bits[3][4] = H264_TAB_CTZ_BITS;
constexpr uint8_t run_len[7][16] = H264_TAB_RUN_LEN, run_bits[7][16] = H264_TAB_RUN_BITS;
}  // namespace vlc_src

constexpr uint16_t vlc_entry(unsigned len, unsigned bits) { return (uint16_t)(len | bits << 8); }
constexpr VlcPacked vlc_packed()
{
    VlcPacked p{};
    for (int t = 0; t < 4; t++)
        for (int i = 0; i < 68; i++) p.e[VLC_CT + 68 * t + i] = vlc_entry(vlc_src::ct_len[t][i], vlc_src::ct_bits[t][i]);
    for (int i = 0; i < 20; i++) p.e[VLC_CDC + i] = vlc_entry(vlc_src::cdc_len[i], vlc_src::cdc_bits[i]);
    for (int t = 0; t < 15; t++)
        for (int i = 0; i < 16; i++) p.e[VLC_TZ + 16 * t + i] = vlc_entry(vlc_src::tz_len[t][i], vlc_src::tz_bits[t][i]);
    for (int t = 0; t < 3; t++)
        for (int i = 0; i < 4; i++) p.e[VLC_CTZ + 4 * t + i] = vlc_entry(vlc_src::ctz_len[t][i], vlc_src::ctz_bits[t][i]);
    for (int t = 0; t < 7; t++)
        for (int i = 0; i < 16; i++) p.e[VLC_RUN + 16 * t + i] = vlc_entry(vlc_src::run_len[t][i], vlc_src::run_bits[t][i]);
    return p;
}
// every entry against the separate arrays (a flat view of each: entry i of table `at` with `n` entries)
constexpr bool vlc_same(const VlcPacked& p, int at, const uint8_t* len, const uint8_t* bits, int n)
{
    for (int i = 0; i < n; i++)
        if ((p.e[at + i] & 255) != len[i] || (p.e[at + i] >> 8) != bits[i]) return false;
    return true;
}
constexpr bool vlc_packed_matches()
{
    constexpr VlcPacked p = vlc_packed();
    for (int t = 0; t < 4; t++)
        if (!vlc_same(p, VLC_CT + 68 * t, vlc_src::ct_len[t], vlc_src::ct_bits[t], 68)) return false;
    if (!vlc_same(p, VLC_CDC, vlc_src::cdc_len, vlc_src::cdc_bits, 20)) return false;
    for (int t = 0; t < 15; t++)
        if (!vlc_same(p, VLC_TZ + 16 * t, vlc_src::tz_len[t], vlc_src::tz_bits[t], 16)) return false;
    for (int t = 0; t < 3; t++)
        if (!vlc_same(p, VLC_CTZ + 4 * t, vlc_src::ctz_len[t], vlc_src::ctz_bits[t], 4)) return false;
    for (int t = 0; t < 7; t++)
        if (!vlc_same(p, VLC_RUN + 16 * t, vlc_src::run_len[t], vlc_src::run_bits[t], 16)) return false;
    return true;
}
static_assert(vlc_packed_matches(), "packed CAVLC tables differ from h264_vlc_tables.h");
static_assert(vlc_packed().e[VLC_CT + 4 * 1 + 1] == vlc_entry(2, 1) && vlc_packed().e[VLC_RUN + 16 * 6 + 14] == vlc_entry(11, 1), "packed CAVLC tables: known entries");

}  // namespace h264
