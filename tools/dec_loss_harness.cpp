// tools/dec_loss_harness.cpp -- media_amd/csrc/dec_loss.h (the arithmetic of the decoder's conceal mode: holes, frame_num gaps, the
// list of ring slots, the damage map) as a stand-alone program on hand-made arrays with known answers.  Built with
// -fsanitize=address,undefined and run by tests/test_dec_loss_host.py; prints "dec_loss ok: N checks" and returns 0, or names the
// first check that failed.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I media_amd/csrc tools/dec_loss_harness.cpp
#include <stdio.h>
#include <string.h>
#include <vector>
#include "dec_loss.h"

using namespace dec_loss;

static int checks = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        checks++;                                                      \
        if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
    } while (0)

// a picture of W x H macroblocks, every macroblock P_L0_16x16 with vector (0, 0), ref_idx 0, one slice, filter off
struct Pic {
    int W, H;
    std::vector<uint8_t> type, refq, avail, conc, out;
    std::vector<int16_t> mv4;
    TaintPic t;
    Pic(int w, int h) : W(w), H(h), type((size_t)w * h, MB_P16), refq((size_t)w * h * 4, 0), avail((size_t)w * h, 0), conc((size_t)w * h, 0), out((size_t)w * h, 0xEE), mv4((size_t)w * h * 32, 0)
    {
        for (int my = 0; my < h; my++)
            for (int mx = 0; mx < w; mx++) {   // one slice, unconstrained intra prediction: bits 0..3 and 4..7 alike
                const int a = (mx > 0 ? 1 : 0) | (my > 0 ? 2 : 0) | (my > 0 && mx + 1 < w ? 4 : 0) | (my > 0 && mx > 0 ? 8 : 0);
                avail[(size_t)my * w + mx] = (uint8_t)(a | (a << 4));
            }
        t.mbw = w; t.mbh = h; t.type = type.data(); t.type_stride = 1; t.mv4 = mv4.data(); t.refq = refq.data(); t.avail = avail.data();
        t.concealed = conc.data(); t.deblock_idc = 1;
    }
    void vec(int mb, int x, int y) { for (int b = 0; b < 16; b++) { mv4[(size_t)mb * 32 + 2 * b] = (int16_t)x; mv4[(size_t)mb * 32 + 2 * b + 1] = (int16_t)y; } }
    int run(int* nconc = nullptr) { return taint_picture(t, out.data(), nconc); }
};

int main()
{
    // ---- holes
    { Hole h = hole_before(0, 8, 24); CHECK(h.from == 0 && h.to == 8); }        // the first slice is missing
    { Hole h = hole_before(8, 8, 24); CHECK(h.from == h.to); }                  // none
    { Hole h = hole_before(8, 16, 24); CHECK(h.from == 8 && h.to == 16); }      // one band in the middle
    { Hole h = hole_before(8, 24, 24); CHECK(h.from == 8 && h.to == 24); }      // two adjacent slices up to the end
    { Hole h = hole_before(16, 99, 24); CHECK(h.to == 24); }                    // never past the picture
    { Hole h = hole_before(16, 8, 24); CHECK(h.from == h.to); }                 // a slice that starts before the expected address is no hole

    // ---- g, across the wrap of frame_num
    CHECK(frame_num_gap(5, 4, 8) == 0);
    CHECK(frame_num_gap(6, 4, 8) == 1);
    CHECK(frame_num_gap(9, 4, 8) == 4);
    CHECK(frame_num_gap(0, 255, 8) == 0);
    CHECK(frame_num_gap(1, 254, 8) == 2);
    CHECK(frame_num_gap(2, 14, 4) == 3);
    CHECK(frame_num_gap(1, 3, 8) == 253);      // a P picture behind a lost IDR picture
    CHECK(frame_num_gap(7, -1, 8) == 0);       // nothing held: nothing can be missing

    // ---- ages
    CHECK(real_age(0, 1) == 0 && real_age(1, 1) == 0 && real_age(2, 1) == 1);
    CHECK(real_age(2, 2) == 0 && real_age(2, 4) == 0 && real_age(2, 0) == 2);
    CHECK(refs_after_gap(1, 1, 3) == 2 && refs_after_gap(3, 1, 3) == 3 && refs_after_gap(1, 4, 3) == 3 && refs_after_gap(1, 253, 1) == 1);

    // ---- the list of slots agrees with real_age: a ring of 4, cur = 2, three held (slots 1, 0, 3)
    for (int g = 1; g <= 4; g++) {
        RefSlots r;
        r.from_ring(2, 3, 4);
        CHECK(r.slot[0] == 1 && r.slot[1] == 0 && r.slot[2] == 3 && !r.standin[0]);
        const int ring[3] = {1, 0, 3};
        r.gap(g);
        for (int a = 0; a < 3; a++) {
            CHECK(r.slot[a] == ring[real_age(a, g)]);
            CHECK((r.standin[a] != 0) == (a < g));
        }
    }
    {   // the window goes on over the list; the next slot is one no held picture lies in
        RefSlots r;
        r.from_ring(2, 3, 4);
        r.gap(1);                                   // 1*, 1, 0
        CHECK(r.next_free(2, 3, 4) == 3);           // cur stays 2 for the picture in hand; behind it 3 is free
        r.push(2, false);                           // 2, 1*, 1
        CHECK(r.slot[0] == 2 && r.slot[1] == 1 && r.standin[1] && r.slot[2] == 1 && !r.standin[2]);
        CHECK(r.next_free(2, 3, 4) == 3);
        r.join(1);
        CHECK(r.slot[0] == 1 && r.slot[2] == 1 && r.standin[0] && r.standin[2] && r.next_free(2, 3, 4) == 3);
        RefSlots one;
        one.from_ring(0, 1, 4);                     // one held picture, in slot 3; ages clamp to it
        CHECK(one.slot[0] == 3 && one.slot[1] == 3 && one.slot[2] == 3);
    }

    // ---- the damage map.  4 x 3 macroblocks; `ref` is the map of the reference picture
    std::vector<uint8_t> clean(12, 0), ref(12, 0);
    ref[5] = TAINTED;                               // macroblock (1, 1)
    {   // a clean reference picture, nothing concealed: clean (negative for every inter rule)
        Pic p(4, 3); p.t.ref[0] = clean.data();
        CHECK(p.run() == 0);
        for (uint8_t v : p.out) CHECK(v == 0);
    }
    {   // concealed macroblocks are tainted and counted
        Pic p(4, 3); p.t.ref[0] = clean.data(); p.conc[2] = p.conc[3] = 1;
        int n = 0;
        CHECK(p.run(&n) == 2 && n == 2 && p.out[2] == (TAINTED | CONCEALED) && p.out[1] == 0);
    }
    {   // a stand-in reference picture taints every inter macroblock; I_PCM stays clean
        Pic p(4, 3); p.type[0] = MB_IPCM;
        CHECK(p.run() == 11 && p.out[0] == 0);
    }
    {   // zero vectors: exactly the macroblock over the tainted one
        Pic p(4, 3); p.t.ref[0] = ref.data();
        CHECK(p.run() == 1 && p.out[5] == TAINTED);
    }
    {   // an integer vector of one macroblock to the left: (2, 1) reads (1, 1); a whole-sample vector needs no margin
        Pic p(4, 3); p.t.ref[0] = ref.data(); p.vec(6, -64, 0); p.vec(5, -64, 0);
        CHECK(p.run() == 1 && p.out[6] == TAINTED && p.out[5] == 0);
    }
    {   // the six-tap margin: a vector of a quarter sample reads 2 columns before and 3 behind; (2, 1) then reads columns 30 .. 50
        Pic p(4, 3); p.t.ref[0] = ref.data(); p.vec(6, 1, 0);
        CHECK(p.run() == 2 && p.out[6] == TAINTED);
        Pic q(4, 3); q.t.ref[0] = ref.data(); q.vec(6, 4, 0);      // one whole sample to the right: columns 33 .. 48, no margin
        CHECK(q.run() == 1 && q.out[6] == 0);
        Pic r(4, 3); r.t.ref[0] = ref.data(); r.vec(9, 0, 2);      // (1, 2), half a sample down: rows 30 .. 51 of the reference
        CHECK(r.run() == 2 && r.out[9] == TAINTED);
        Pic s(4, 3); s.t.ref[0] = ref.data(); s.vec(4, -3, 0);     // (0, 1), 3/4 sample left: columns -3 .. 18, clamped, reach (1, 1)
        CHECK(s.run() == 2 && s.out[4] == TAINTED);
    }
    {   // chroma: a vector of one whole luma sample is half a chroma sample, and the chroma block reads one sample more
        Pic p(4, 3); p.t.ref[0] = ref.data(); p.vec(6, -4, 0);     // (2, 1), one luma column left: luma column 31 is (1, 1)'s
        CHECK(p.run() == 2);
        Pic q(4, 3); q.t.ref[0] = ref.data(); q.vec(9, 0, 4);      // (1, 2), one luma row down: luma rows 33 .. 48, chroma rows 16 .. 24: clean
        CHECK(q.run() == 1 && q.out[9] == 0);
        Pic r(4, 3); r.t.ref[0] = ref.data(); r.vec(9, 0, -4);     // one luma row up: luma row 31 is (1, 1)'s
        CHECK(r.run() == 2 && r.out[9] == TAINTED);
    }
    {   // clamping: a vector far outside reads the border macroblock
        std::vector<uint8_t> corner(12, 0); corner[0] = TAINTED;
        Pic p(4, 3); p.t.ref[0] = corner.data(); p.vec(7, -4000, -4000);
        CHECK(p.run() == 2 && p.out[7] == TAINTED);
    }
    {   // the reference index chooses the map
        Pic p(4, 3); p.t.ref[0] = clean.data(); p.t.ref[1] = ref.data();
        for (int q = 0; q < 4; q++) p.refq[5 * 4 + q] = 1;
        CHECK(p.run() == 1 && p.out[5] == TAINTED);
        p.t.ref[1] = nullptr;
        CHECK(p.run() == 1);
    }
    {   // intra: tainted by a neighbour A, B, C or D its prediction may read - positive for each, negative without the bit
        const int at[4] = {4, 1, 2, 0}, bit[4] = {16, 32, 64, 128};   // the neighbours of (1, 1): left, above, above-right, above-left
        for (int n = 0; n < 4; n++) {
            Pic p(4, 3); p.t.ref[0] = clean.data(); p.type[5] = MB_I4; p.conc[at[n]] = 1;
            CHECK(p.run() == 2 && p.out[5] == TAINTED);
            Pic q(4, 3); q.t.ref[0] = clean.data(); q.type[5] = MB_I16; q.conc[at[n]] = 1;
            q.avail[5] = (uint8_t)(q.avail[5] & ~bit[n]);              // another slice, or an inter macroblock under constrained_intra_pred
            CHECK(q.run() == 1 && q.out[5] == 0);
        }
        Pic r(4, 3); r.t.ref[0] = clean.data(); r.type[5] = MB_I16; r.conc[6] = 1;   // the macroblock to the RIGHT is no neighbour
        CHECK(r.run() == 1 && r.out[5] == 0);
    }
    {   // the filter.  idc 1: no edge; idc 0: every edge in the picture, and on along the decoding order; idc 2: not across slices
        Pic p(4, 3); p.t.ref[0] = clean.data(); p.conc[5] = 1; p.t.deblock_idc = 1;
        CHECK(p.run() == 1);
        p.t.deblock_idc = 0;   // (1, 1): its left and top neighbours by its own edges; (2, 1) by its left edge, and with it (2, 0) by its
                               // top edge; so on along the decoding order: only (0, 0) stays clean
        CHECK(p.run() == 11 && p.out[4] == TAINTED && p.out[1] == TAINTED && p.out[0] == 0 && p.out[2] == TAINTED && p.out[6] == TAINTED && p.out[11] == TAINTED);
        p.t.deblock_idc = 2;   // one slice: the same
        CHECK(p.run() == 11);
        for (int mx = 0; mx < 4; mx++) { p.avail[4 + mx] &= (uint8_t)~(2 | 4 | 8); p.avail[8 + mx] &= (uint8_t)~(2 | 4 | 8); }   // three slices of one row
        CHECK(p.run() == 4 && p.out[1] == 0 && p.out[9] == 0 && p.out[4] == TAINTED && p.out[7] == TAINTED);
        p.t.deblock_idc = 0;   // edges between slices are filtered
        CHECK(p.run() == 11);
    }
    {   // an IDR picture whose slices were all received resets the map: all intra, nothing concealed, whatever the references were
        Pic p(4, 3);
        for (auto& t : p.type) t = MB_I16;
        p.type[7] = MB_I4; p.t.deblock_idc = 0;
        CHECK(p.run() == 0);
        for (uint8_t v : p.out) CHECK(v == 0);
    }
    printf("dec_loss ok: %d checks\n", checks);
    return 0;
}
