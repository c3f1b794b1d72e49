// tools/damage_harness.cpp -- media_amd/csrc/damage.h alone, under AddressSanitizer + UBSan (tests/test_damage_host.py builds and
// runs it):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I media_amd/csrc tools/damage_harness.cpp
// Random sizes, layouts, strides, rectangles and changes.  Every caller plane is allocated to its exact size - (rows - 1) * stride +
// row bytes, the padding behind the last row not included - so that a read of the last row's padding or past the picture is caught;
// the padding between rows holds noise that changes from picture to picture, so that a compare that reads it marks tiles the brute
// force does not.  Checked against a per-byte brute force written here: the tile set of rectangles and of detect, the twin after
// the call (the stated composition; with detect the caller's picture), the payload's header, indices, size and padding, that
// applying the payload to the old slot gives the twin, and the fallback rule at its boundary.  Aborts on the first difference.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <set>

#include "damage.h"

using namespace damage;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "damage_harness: line %d: %s\n", __LINE__, #c); abort(); } } while (0)

static std::mt19937 rng(12345);
static int rnd(int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); }

struct Caller {   // a caller's picture: planes of their exact size, rows a stride apart
    int layout, w, h, nplanes;
    std::unique_ptr<uint8_t[]> mem[3];
    int stride[3], rows[3];
    size_t rowb[3];
    Picture pic() const { return Picture{layout, {mem[0].get(), mem[1].get(), mem[2].get()}, {stride[0], stride[1], stride[2]}}; }
    uint8_t& at(int p, int r, size_t x) { return mem[p][(size_t)r * stride[p] + x]; }
};

static Caller make_caller(int layout, int w, int h, bool tight)
{
    Caller c;
    c.layout = layout; c.w = w; c.h = h;
    c.nplanes = layout == LAYOUT_RGBA ? 1 : layout == LAYOUT_NV12 ? 2 : 3;
    for (int p = 0; p < 3; p++) { c.stride[p] = 0; c.rows[p] = 0; c.rowb[p] = 0; }
    for (int p = 0; p < c.nplanes; p++) {
        c.rowb[p] = tight_row_bytes(layout, w, p);
        c.rows[p] = p ? h / 2 : h;
        c.stride[p] = (int)c.rowb[p] + (tight ? 0 : rnd(0, 19));
        const size_t n = (size_t)(c.rows[p] - 1) * c.stride[p] + c.rowb[p];
        c.mem[p].reset(new uint8_t[n]);
        for (size_t i = 0; i < n; i++) c.mem[p][i] = (uint8_t)rng();
    }
    return c;
}

static void noise_in_padding(Caller& c)
{
    for (int p = 0; p < c.nplanes; p++)
        for (int r = 0; r + 1 < c.rows[p]; r++)
            for (size_t x = c.rowb[p]; x < (size_t)c.stride[p]; x++) c.at(p, r, x) = (uint8_t)rng();
}

static std::vector<uint8_t> tight_of(Caller& c)
{
    std::vector<uint8_t> t(picture_bytes(c.layout, c.w, c.h));
    for (int p = 0; p < c.nplanes; p++)
        for (int r = 0; r < c.rows[p]; r++) memcpy(t.data() + tight_offset(c.layout, c.w, c.h, p, r, 0), &c.at(p, r, 0), c.rowb[p]);
    return t;
}

// the tile of byte i of a tight picture, from the definition: its plane, row and column -> luma position -> tile
static int tile_of_byte(int layout, int w, int h, size_t i)
{
    const size_t ysz = (size_t)w * h;
    int lx, ly;
    if (layout == LAYOUT_RGBA) { ly = (int)(i / ((size_t)w * 4)); lx = (int)(i % ((size_t)w * 4)) / 4; }
    else if (i < ysz) { ly = (int)(i / w); lx = (int)(i % w); }
    else if (layout == LAYOUT_NV12) { const size_t j = i - ysz; ly = 2 * (int)(j / w); lx = (int)(j % w); }
    else { const size_t j = (i - ysz) % (ysz / 4); ly = 2 * (int)(j / (w / 2)); lx = 2 * (int)(j % (w / 2)); }
    return (ly / TILE_H) * tiles_x(w) + lx / TILE_W;
}

static void one_round(int layout, int w, int h)
{
    const int nt = tiles_total(w, h), ntx = tiles_x(w);
    const size_t pb = picture_bytes(layout, w, h);
    Caller c = make_caller(layout, w, h, rnd(0, 3) == 0);
    std::vector<uint8_t> twin = tight_of(c);   // the slot's pinned twin after a whole upload
    std::unique_ptr<uint8_t[]> twin_exact(new uint8_t[pb]), slot(new uint8_t[pb]);
    for (int pic = 0; pic < 6; pic++) {
        // change a few bytes of the caller's picture (sometimes none, sometimes all), and all of the padding
        const int kind = rnd(0, 5);
        const int nchange = kind == 0 ? 0 : kind == 1 ? -1 : rnd(1, 6);
        for (int p = 0; p < c.nplanes; p++)
            for (int r = 0; r < c.rows[p]; r++)
                for (size_t x = 0; x < c.rowb[p]; x++)
                    if (nchange < 0 || (nchange > 0 && rnd(0, (int)pb / nchange) == 0)) c.at(p, r, x) = (uint8_t)(c.at(p, r, x) + 1 + rng() % 255);
        noise_in_padding(c);
        const std::vector<uint8_t> now = tight_of(c), before = twin;
        std::set<int> brute;
        for (size_t i = 0; i < pb; i++) if (now[i] != before[i]) brute.insert(tile_of_byte(layout, w, h, i));
        memcpy(twin_exact.get(), before.data(), pb);   // (its own allocation of the exact size: a write past the twin is caught)
        memcpy(slot.get(), before.data(), pb);
        std::vector<uint8_t> mark;
        std::set<int> want;
        const bool detect = rnd(0, 1) == 0;
        if (detect) {
            detect_and_copy(c.pic(), w, h, twin_exact.get(), mark);
            want = brute;
            CHECK(!memcmp(twin_exact.get(), now.data(), pb));
        } else {
            std::vector<Rect> rects((size_t)rnd(0, 4));
            for (Rect& r : rects) r = Rect{rnd(-20, w + 10), rnd(-20, h + 10), rnd(0, w), rnd(0, h)};
            if (!rects.empty() && rnd(0, 3) == 0) rects[0] = Rect{INT32_MAX - 3, INT32_MAX - 3, INT32_MAX, INT32_MAX};   // (no overflow)
            if (!rects.empty() && rnd(0, 5) == 0) rects[0] = Rect{-100, -100, 100000, 100000};
            CHECK(rects_to_tiles(w, h, rects.data(), (int)rects.size(), mark));
            for (const Rect& r : rects)
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++)
                        if ((int64_t)x >= r.x && (int64_t)x < (int64_t)r.x + r.w && (int64_t)y >= r.y && (int64_t)y < (int64_t)r.y + r.h) want.insert((y / TILE_H) * ntx + x / TILE_W);
            copy_tiles(c.pic(), w, h, mark, twin_exact.get());
            for (size_t i = 0; i < pb; i++) CHECK(twin_exact[i] == (want.count(tile_of_byte(layout, w, h, i)) ? now[i] : before[i]));
        }
        CHECK((int)mark.size() == nt);
        for (int t = 0; t < nt; t++) CHECK((mark[(size_t)t] != 0) == (want.count(t) != 0));
        const size_t n = count_tiles(mark);
        CHECK(n == want.size());
        // the payload: its own allocation of exactly payload_bytes
        const size_t bytes = payload_bytes(layout, n);
        CHECK(bytes == ((16 + 4 * n + 15) / 16) * 16 + n * (layout == LAYOUT_RGBA ? 4096u : 1536u));
        std::unique_ptr<uint8_t[]> pay(new uint8_t[bytes]);
        memset(pay.get(), 0xA5, bytes);
        CHECK(pack_payload(layout, w, h, twin_exact.get(), mark, pay.get()) == bytes);
        Header hd;
        memcpy(&hd, pay.get(), sizeof(hd));
        CHECK(hd.magic == MAGIC && hd.layout == (uint32_t)layout && hd.ntiles == n && hd.tile_bytes == tile_bytes(layout));
        size_t k = 0;
        for (int t : want) { uint32_t idx; memcpy(&idx, pay.get() + 16 + 4 * k++, 4); CHECK(idx == (uint32_t)t); }
        for (size_t i = 16 + 4 * n; i < tiles_offset(n); i++) CHECK(pay[i] == 0);
        apply_payload(w, h, pay.get(), slot.get());
        CHECK(!memcmp(slot.get(), twin_exact.get(), pb));
        const int mode = upload_mode(layout, w, h, n);
        CHECK(mode == (n == 0 ? MODE_NOTHING : bytes < pb ? MODE_PATCHED : MODE_WHOLE));
        twin.assign(twin_exact.get(), twin_exact.get() + pb);
    }
}

int main()
{
    // what is refused, and that nothing is marked then
    std::vector<uint8_t> mark;
    const Rect bad_w{0, 0, -1, 4}, bad_h{0, 0, 4, -1}, good{0, 0, 4, 4};
    CHECK(!rects_to_tiles(66, 34, &good, -1, mark) && !rects_to_tiles(66, 34, nullptr, 1, mark) && !rects_to_tiles(66, 34, &bad_w, 1, mark) && !rects_to_tiles(66, 34, &bad_h, 1, mark));
    CHECK(mark.empty());
    const Rect two[2] = {good, bad_h};
    CHECK(!rects_to_tiles(66, 34, two, 2, mark) && mark.empty());
    CHECK(rects_to_tiles(66, 34, nullptr, 0, mark) && mark.size() == 6 && count_tiles(mark) == 0);
    // the boundary of the fallback rule, one tile under and one over
    for (int layout = 0; layout < 3; layout++) {
        const int sizes[5][2] = {{34, 18}, {66, 34}, {128, 48}, {320, 240}, {1920, 1080}};
        for (const auto& s : sizes) {
            size_t n = 0;
            while (payload_bytes(layout, n + 1) < picture_bytes(layout, s[0], s[1])) n++;
            CHECK(upload_mode(layout, s[0], s[1], n) == (n ? MODE_PATCHED : MODE_NOTHING) && upload_mode(layout, s[0], s[1], n + 1) == MODE_WHOLE);
        }
    }
    CHECK(parse_mode_key(nullptr) == 0 && parse_mode_key("") == 0 && parse_mode_key("off") == 0 && parse_mode_key("detect") == 1);
    CHECK(parse_mode_key("on") == -1 && parse_mode_key("Detect") == -1 && parse_mode_key("detect ") == -1 && parse_mode_key("1") == -1);
    const int sizes[][2] = {{34, 18}, {66, 34}, {128, 48}, {16, 16}, {64, 16}, {130, 50}, {34, 66}, {192, 32}, {322, 242}};
    int rounds = 0;
    for (int rep = 0; rep < 6; rep++)
        for (const auto& s : sizes)
            for (int layout = 0; layout < 3; layout++) { one_round(layout, s[0], s[1]); rounds++; }
    for (int rep = 0; rep < 40; rep++) { one_round(rnd(0, 2), 2 * rnd(8, 100), 2 * rnd(8, 60)); rounds++; }
    printf("ok damage: %d rounds of 6 pictures\n", rounds);
    return 0;
}
