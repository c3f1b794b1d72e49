// tools/pic_seq_harness.cpp -- the picture-sequence rule of media_amd/csrc/host_framing.h alone (PicSeq, slice_nal_hdr,
// build_slice_header; no HIP, any host compiler):
//   g++ -std=c++17 -O1 -o pic_seq_harness tools/pic_seq_harness.cpp
//   pic_seq_harness LAYERS GOP REFS SLICES QP SCRIPT
// SCRIPT holds one letter per picture: '.' a picture, 'I' an IDR picture is forced before it, 'F' the picture fails (it does not go
// out: the stream hub's rule - nothing moves, the next picture is an IDR picture).  One line per picture:
//   idr layer ring-slot frame_num reference-count nal-header-byte me-facts last-slot slice-header-bits
// driven as engine.h and hub_sched.h drive the struct: next_is_idr, begin, (the picture), advance or force_idr.
// tests/test_temporal_host.py compares the lines with the restatement in tests/temporal.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../media_amd/csrc/host_framing.h"

int main(int argc, char** argv)
{
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
            const int k = seq.refresh_band(idr);
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
        const int layer = seq.layer(), nref = seq.avail_refs(idr, nrefs);
        uint64_t bits = 0;
        const int n = build_slice_header(shape, idr, seq.idr_id, false, seq.frame_num, qp, nref, &bits, layer != 0);
        printf("%d %d %d %d %d %d %d ", idr ? 1 : 0, layer, seq.cur, seq.frame_num, nref, slice_nal_hdr(idr, layer), seq.me_facts(idr));
        const int slot = seq.cur;
        if (*p == 'F') seq.force_idr = 1;
        else seq.advance(idr, nbuf, 1);
        printf("%d ", *p == 'F' ? -1 : seq.last_slot(nbuf) == slot ? slot : -2);
        for (int i = n - 1; i >= 0; i--) putchar('0' + (int)((bits >> i) & 1));
        putchar('\n');
    }
    return 0;
}
