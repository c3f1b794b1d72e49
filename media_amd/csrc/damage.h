// media_amd/csrc/damage.h -- damage tiles of a host-fed stream (include/mi355x_h264.h, "damage tiles"), without HIP and without the
// hub (tools/damage_harness.cpp drives this file alone under AddressSanitizer + UBSan): the tile grid, rectangles -> tile set, the
// fused compare-and-copy of detect mode, the payload a damage call puts on the link, and the rule that sends a call the ordinary
// way.  tests/damage.py restates all of it in numpy.
//
// Grid: tiles of 64 x 16 luma samples at multiples of (64, 16) over the SOURCE picture w x h (both even); tile t = ty * tiles_x + tx.
// Tiles at the right and bottom edge are partial.  A tile's bytes, at its full nominal size (offsets inside the tile):
//   I420  [0, 1024) Y 16 rows of 64   [1024, 1280) U 8 rows of 32   [1280, 1536) V 8 rows of 32
//   NV12  [0, 1024) Y 16 rows of 64   [1024, 1536) UV 8 rows of 64
//   RGBA  [0, 4096) 16 rows of 256
// Payload: Header (16 bytes), ntiles uint32 tile indices (ascending), zero padding to a multiple of 16, then the tiles in the order of
// the list.  Bytes of a partial tile that lie outside the picture are never written here and never stored on the device.
// Rule: a call goes patched when 0 < payload_bytes(layout, ntiles) < picture_bytes(layout, w, h); with payload_bytes >= picture_bytes
// it goes whole; with no tile nothing goes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace damage {

enum { TILE_W = 64, TILE_H = 16, HEADER_BYTES = 16 };
enum { LAYOUT_I420 = 0, LAYOUT_NV12 = 1, LAYOUT_RGBA = 2 };
enum { MODE_WHOLE = 0, MODE_PATCHED = 1, MODE_NOTHING = 2, MODE_IN_PLACE = 3 };   // MI355X_H264_UPLOAD_*
const uint32_t MAGIC = 0x474D4144u;   // "DAMG"

struct Rect { int32_t x, y, w, h; };                              // mi355x_h264_rect
struct Header { uint32_t magic, layout, ntiles, tile_bytes; };
struct Picture { int layout; const uint8_t* p[3]; int stride[3]; };   // the caller's planes, rows stride[k] bytes apart
static_assert(sizeof(Header) == HEADER_BYTES && sizeof(Rect) == 16, "layouts");

inline int tiles_x(int w) { return (w + TILE_W - 1) / TILE_W; }
inline int tiles_y(int h) { return (h + TILE_H - 1) / TILE_H; }
inline int tiles_total(int w, int h) { return tiles_x(w) * tiles_y(h); }
inline size_t tile_bytes(int layout) { return layout == LAYOUT_RGBA ? (size_t)TILE_W * TILE_H * 4 : (size_t)TILE_W * TILE_H * 3 / 2; }
inline size_t picture_bytes(int layout, int w, int h) { return layout == LAYOUT_RGBA ? (size_t)w * h * 4 : (size_t)w * h * 3 / 2; }
inline size_t tiles_offset(size_t ntiles) { return (HEADER_BYTES + 4 * ntiles + 15) & ~(size_t)15; }
inline size_t payload_bytes(int layout, size_t ntiles) { return tiles_offset(ntiles) + ntiles * tile_bytes(layout); }
inline int upload_mode(int layout, int w, int h, size_t ntiles)
{
    return ntiles == 0 ? MODE_NOTHING : payload_bytes(layout, ntiles) < picture_bytes(layout, w, h) ? MODE_PATCHED : MODE_WHOLE;
}

// The row segments of tile (tx, ty) that lie inside the picture: f(plane, row, x, len, off) - `len` bytes at byte x of row `row` of
// the caller's plane `plane`, which lie at tight + tight_offset(plane, row, x) in a tight picture and at `off` inside the tile.
template <class F>
inline void tile_segments(int layout, int w, int h, int tx, int ty, F&& f)
{
    const int x0 = tx * TILE_W, y0 = ty * TILE_H;
    const int cw = w - x0 < TILE_W ? w - x0 : TILE_W, rh = h - y0 < TILE_H ? h - y0 : TILE_H;
    if (layout == LAYOUT_RGBA) {
        for (int r = 0; r < rh; r++) f(0, y0 + r, (size_t)x0 * 4, (size_t)cw * 4, (size_t)r * TILE_W * 4);
        return;
    }
    for (int r = 0; r < rh; r++) f(0, y0 + r, (size_t)x0, (size_t)cw, (size_t)r * TILE_W);
    const size_t c0 = (size_t)TILE_W * TILE_H;
    if (layout == LAYOUT_NV12) {
        for (int r = 0; r < rh / 2; r++) f(1, y0 / 2 + r, (size_t)x0, (size_t)cw, c0 + (size_t)r * TILE_W);
        return;
    }
    for (int p = 1; p <= 2; p++)
        for (int r = 0; r < rh / 2; r++) f(p, y0 / 2 + r, (size_t)x0 / 2, (size_t)cw / 2, c0 + (size_t)(p - 1) * (TILE_W / 2) * (TILE_H / 2) + (size_t)r * (TILE_W / 2));
}

inline size_t tight_row_bytes(int layout, int w, int plane) { return layout == LAYOUT_RGBA ? (size_t)w * 4 : plane && layout == LAYOUT_I420 ? (size_t)w / 2 : (size_t)w; }
inline size_t tight_offset(int layout, int w, int h, int plane, int row, size_t x)
{
    const size_t ysz = (size_t)w * h;
    return (plane == 0 ? 0 : plane == 1 ? ysz : ysz + ysz / 4) + (size_t)row * tight_row_bytes(layout, w, plane) + x;
}

// Caller rectangles -> tile marks (mark[t] = 1; marks already set stay).  Rectangles are clipped to the picture; an empty one or one
// wholly outside adds nothing.  false: n < 0, n > 0 with null rects, or a negative width or height - nothing was marked.
inline bool rects_to_tiles(int w, int h, const Rect* rects, int n, std::vector<uint8_t>& mark)
{
    if (n < 0 || (n > 0 && !rects)) return false;
    for (int i = 0; i < n; i++) if (rects[i].w < 0 || rects[i].h < 0) return false;
    const int ntx = tiles_x(w);
    mark.resize((size_t)tiles_total(w, h), 0);
    for (int i = 0; i < n; i++) {
        const int64_t xa = rects[i].x < 0 ? 0 : rects[i].x, ya = rects[i].y < 0 ? 0 : rects[i].y;
        int64_t xb = (int64_t)rects[i].x + rects[i].w, yb = (int64_t)rects[i].y + rects[i].h;   // (exclusive)
        if (xb > w) xb = w;
        if (yb > h) yb = h;
        if (xa >= xb || ya >= yb) continue;
        for (int64_t ty = ya / TILE_H; ty <= (yb - 1) / TILE_H; ty++)
            for (int64_t tx = xa / TILE_W; tx <= (xb - 1) / TILE_W; tx++) mark[(size_t)(ty * ntx + tx)] = 1;
    }
    return true;
}

// the marked tiles of the caller's picture into the tight picture `tight` (the pinned twin of the stream's slot)
inline void copy_tiles(const Picture& in, int w, int h, const std::vector<uint8_t>& mark, uint8_t* tight)
{
    const int ntx = tiles_x(w), nty = tiles_y(h);
    for (int ty = 0; ty < nty; ty++)
        for (int tx = 0; tx < ntx; tx++)
            if (mark[(size_t)ty * ntx + tx])
                tile_segments(in.layout, w, h, tx, ty, [&](int p, int row, size_t x, size_t len, size_t) {
                    memcpy(tight + tight_offset(in.layout, w, h, p, row, x), in.p[p] + (size_t)row * in.stride[p] + x, len);
                });
}

// Detect mode, compare and copy in one walk: mark[t] = 1 for every tile with a byte inside the picture that differs from `tight`,
// and those tiles are copied into `tight`, which then equals the caller's picture.  A band of tile rows at a time: whole picture
// rows are compared first (an unchanged row costs one memcmp), only rows that differ are looked at per tile.  The caller's stride
// padding is never read.
inline void detect_and_copy(const Picture& in, int w, int h, uint8_t* tight, std::vector<uint8_t>& mark)
{
    const int ntx = tiles_x(w), nty = tiles_y(h), L = in.layout;
    const int nplanes = L == LAYOUT_RGBA ? 1 : L == LAYOUT_NV12 ? 2 : 3;
    mark.assign((size_t)ntx * nty, 0);
    for (int ty = 0; ty < nty; ty++) {
        uint8_t* const m = mark.data() + (size_t)ty * ntx;
        const int y0 = ty * TILE_H, rh = h - y0 < TILE_H ? h - y0 : TILE_H;
        int marked = 0;
        for (int p = 0; p < nplanes && marked < ntx; p++) {
            const size_t rb = tight_row_bytes(L, w, p);
            const size_t seg = L == LAYOUT_RGBA ? (size_t)TILE_W * 4 : p && L == LAYOUT_I420 ? (size_t)TILE_W / 2 : (size_t)TILE_W;   // a tile's bytes of a row
            const int r0 = p ? y0 / 2 : y0, nr = p ? rh / 2 : rh;
            for (int r = r0; r < r0 + nr && marked < ntx; r++) {
                const uint8_t* const a = in.p[p] + (size_t)r * in.stride[p];
                const uint8_t* const b = tight + tight_offset(L, w, h, p, r, 0);
                if (!memcmp(a, b, rb)) continue;
                for (int tx = 0; tx < ntx; tx++) {
                    if (m[tx]) continue;
                    const size_t o = (size_t)tx * seg, len = rb - o < seg ? rb - o : seg;
                    if (memcmp(a + o, b + o, len)) { m[tx] = 1; marked++; }
                }
            }
        }
        if (!marked) continue;
        for (int tx = 0; tx < ntx; tx++)
            if (m[tx])
                tile_segments(L, w, h, tx, ty, [&](int p, int row, size_t x, size_t len, size_t) {
                    memcpy(tight + tight_offset(L, w, h, p, row, x), in.p[p] + (size_t)row * in.stride[p] + x, len);
                });
    }
}

inline size_t count_tiles(const std::vector<uint8_t>& mark) { size_t n = 0; for (uint8_t v : mark) n += v; return n; }

// The payload of the marked tiles, read from the tight picture (which holds them already): header, indices, padding, tiles.  `out`
// has room for payload_bytes(layout, count_tiles(mark)); returns that number.
inline size_t pack_payload(int layout, int w, int h, const uint8_t* tight, const std::vector<uint8_t>& mark, uint8_t* out)
{
    const size_t n = count_tiles(mark), tb = tile_bytes(layout), toff = tiles_offset(n);
    const Header hd{MAGIC, (uint32_t)layout, (uint32_t)n, (uint32_t)tb};
    memcpy(out, &hd, sizeof(hd));
    memset(out + HEADER_BYTES + 4 * n, 0, toff - HEADER_BYTES - 4 * n);
    const int ntx = tiles_x(w);
    size_t k = 0;
    for (size_t t = 0; t < mark.size(); t++) {
        if (!mark[t]) continue;
        const uint32_t idx = (uint32_t)t;
        memcpy(out + HEADER_BYTES + 4 * k, &idx, 4);
        uint8_t* const tile = out + toff + k * tb;
        tile_segments(layout, w, h, (int)(t % ntx), (int)(t / ntx), [&](int p, int row, size_t x, size_t len, size_t off) {
            memcpy(tile + off, tight + tight_offset(layout, w, h, p, row, x), len);
        });
        k++;
    }
    return toff + n * tb;
}

// what k_patch_step does, on the host (the harness checks pack -> apply against the composition): the payload's tiles into `slot`
inline void apply_payload(int w, int h, const uint8_t* payload, uint8_t* slot)
{
    Header hd;
    memcpy(&hd, payload, sizeof(hd));
    const size_t toff = tiles_offset(hd.ntiles);
    const int ntx = tiles_x(w);
    for (uint32_t k = 0; k < hd.ntiles; k++) {
        uint32_t t;
        memcpy(&t, payload + HEADER_BYTES + 4 * (size_t)k, 4);
        const uint8_t* const tile = payload + toff + (size_t)k * hd.tile_bytes;
        tile_segments((int)hd.layout, w, h, (int)(t % ntx), (int)(t / ntx), [&](int p, int row, size_t x, size_t len, size_t off) {
            memcpy(slot + tight_offset((int)hd.layout, w, h, p, row, x), tile + off, len);
        });
    }
}

// persist.vmi.video.encode.damage: "off" (and unset / empty) -> 0, "detect" -> 1, anything else -> -1 (refused)
inline int parse_mode_key(const char* v)
{
    if (!v || !v[0] || !strcmp(v, "off")) return 0;
    return !strcmp(v, "detect") ? 1 : -1;
}

}  // namespace damage
