// tools/pic_seq_harness.cpp -- the picture-sequence rule of media_amd/csrc/host_framing.h alone (PicSeq and the record PicSeq::pic
// makes of a picture, slice_nal_hdr, build_slice_header) and the device words of item_word.h; no HIP, any host compiler:
//   g++ -std=c++17 -O1 -o pic_seq_harness tools/pic_seq_harness.cpp
//   pic_seq_harness LAYERS GOP REFS SLICES QP SCRIPT
// SCRIPT holds one letter per picture: '.' a picture, 'I' an IDR picture is forced before it, 'F' the picture fails (it does not go
// out: the stream hub's rule - nothing moves, the next picture is an IDR picture).  One line per picture:
//   idr layer ring-slot frame_num reference-count nal-header-byte me-facts last-slot slice-header-bits
// driven as engine.h and hub_sched.h drive the struct: next_is_idr, begin, pic (the picture), advance or force_idr.
// tests/test_temporal_host.py compares the lines with the restatement in tests/temporal.py.
//   pic_seq_harness words LAYERS GOP REFS SLICES REFRESH QP SCRIPT  - REFRESH: bands of an intra refresh stream, 0 = off.  One line per
// picture: idr, the record (item cur qp frame_num idr_id nref layer me rband), item_word in hex, its error flag, me_word, item_unpack
// of the word (item cur nref qp me rband)
//   pic_seq_harness pack ITEM CUR QP NREF ME RBAND  - the three functions of item_word.h on one record, as the tail of a words line
//   pic_seq_harness batch IDR_ID STEP G  - idr_pic_id of the items 0 .. G - 1 of a direct batch (batch_item_pic)
// tests/test_step_record_host.py
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../media_amd/csrc/host_framing.h"

static void print_words(const ItemPic& p, bool refresh)
{
    bool bad = false;
    const uint32_t w = item_word(p, &bad);
    const ItemRef u = item_unpack(w);
    printf("%08x %d %d %d %d %d %d %d %d\n", w, bad ? 1 : 0, me_word(p, refresh), u.item, u.cur, u.nref, u.qp, u.me, u.rband);
}

int main(int argc, char** argv)
{
    if (argc == 9 && !strcmp(argv[1], "words")) {
        const int gop = atoi(argv[3]), nrefs = std::max(1, atoi(argv[4])), qp = atoi(argv[7]);
        PicSeq seq;
        seq.layers = atoi(argv[2]); seq.refresh_n = atoi(argv[6]);
        for (const char* p = argv[8]; *p; p++) {
            if (*p == 'I') seq.force_idr = 1;
            const bool idr = seq.next_is_idr(gop);
            seq.begin(idr);
            const ItemPic pic = seq.pic(0, qp, idr, nrefs);
            printf("%d %d %d %d %d %d %d %d %d %d ", idr ? 1 : 0, pic.item, pic.cur, pic.qp, pic.frame_num, pic.idr_id, pic.nref, pic.layer, pic.me, pic.rband);
            print_words(pic, seq.refresh_n != 0);
            if (*p == 'F') seq.force_idr = 1;
            else seq.advance(idr, nrefs + 1, 1);
        }
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "pack")) {
        print_words(ItemPic{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), 0, 0, atoi(argv[5]), 0, atoi(argv[6]), atoi(argv[7])}, true);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "batch")) {
        PicSeq seq;
        seq.idr_id = atoi(argv[2]) & 0xFF;
        seq.begin(true);
        for (int g = 0; g < atoi(argv[4]); g++) {
            const ItemPic pic = batch_item_pic(seq.pic(0, 26, true, 1), g, atoi(argv[3]));
            printf("%d %d\n", pic.item, pic.idr_id);
        }
        return 0;
    }
    // intra refresh:  pic_seq_harness refresh N GOP SCRIPT  - one line per picture: idr p k sei-bytes-in-hex ('-' where the access unit
    // has none); SCRIPT as above.  pic_seq_harness bands MBH SLICES - refresh_bands().  tests/test_intra_refresh_host.py
    if (argc == 5 && !strcmp(argv[1], "refresh")) {
        const int n = atoi(argv[2]), gop = atoi(argv[3]);
        PicSeq seq;
        seq.refresh_n = n;
        for (const char* p = argv[4]; *p; p++) {
            if (*p == 'I') seq.force_idr = 1;
            const bool idr = seq.next_is_idr(gop);
            seq.begin(idr);
            const int k = seq.pic(0, 26, idr, 1).rband;
            printf("%d %d %d ", idr ? 1 : 0, idr ? 0 : seq.refresh_p(), k);
            if (k == 0) {
                std::vector<uint8_t> au;
                append_recovery_point_sei(au, n);
                for (uint8_t v : au) printf("%02x", v);
            } else putchar('-');
            putchar('\n');
            if (*p == 'F') seq.force_idr = 1;
            else seq.advance(idr, 2, 1);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "bands")) { printf("%d\n", refresh_bands(atoi(argv[2]), atoi(argv[3]))); return 0; }
    if (argc != 7) { fprintf(stderr, "usage: %s LAYERS GOP REFS SLICES QP SCRIPT\n", argv[0]); return 2; }
    const int layers = atoi(argv[1]), gop = atoi(argv[2]), nrefs = std::max(1, atoi(argv[3])), nsl = std::max(1, atoi(argv[4])), qp = atoi(argv[5]);
    const char* script = argv[6];
    StreamShape shape{};
    shape.nrefs = nrefs; shape.nsl = nsl; shape.disable_deblock = 0;
    PicSeq seq;
    seq.layers = layers;
    const int nbuf = nrefs + 1;
    for (const char* p = script; *p; p++) {
        if (*p == 'I') seq.force_idr = 1;
        const bool idr = seq.next_is_idr(gop);
        seq.begin(idr);
        const ItemPic pic = seq.pic(0, qp, idr, nrefs);
        uint64_t bits = 0;
        const int n = build_slice_header(shape, idr, pic.idr_id, false, pic.frame_num, pic.qp, pic.nref, &bits, pic.layer != 0);
        printf("%d %d %d %d %d %d %d ", idr ? 1 : 0, pic.layer, pic.cur, pic.frame_num, pic.nref, slice_nal_hdr(idr, pic.layer), pic.me);
        const int slot = seq.cur;
        if (*p == 'F') seq.force_idr = 1;
        else seq.advance(idr, nbuf, 1);
        printf("%d ", *p == 'F' ? -1 : seq.last_slot(nbuf) == slot ? slot : -2);
        for (int i = n - 1; i >= 0; i--) putchar('0' + (int)((bits >> i) & 1));
        putchar('\n');
    }
    return 0;
}
