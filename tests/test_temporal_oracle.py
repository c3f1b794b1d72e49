"""Two temporal layers on the oracle alone (CPU): the composition of tests/temporal.py gives a stream the independent decoder
decodes to the reconstructions named there - whole, and with its non-reference pictures dropped - and the case list holds what
tests/test_gpu_temporal.py needs it to hold.  Nothing of the encoder under test runs here."""
import numpy as np
import pytest
import temporal as tl
from media_amd import temporal as mt
from oracle_lib import OracleDecoder

IDS = [c.name for c in tl.CASES]


def _decode_all(stream_aus):
    dec, out = OracleDecoder(), []
    for au in stream_aus:
        assert dec.decode(au) == 1
        out.append(([dec.plane(p) for p in range(3)], dec.last_is_ref))
    dec.close()
    return out


@pytest.mark.parametrize("c", tl.CASES, ids=IDS)
def test_composed_stream_decodes_whole_and_as_base_layer(c):
    """fact C: every picture of the composed stream decodes to the reconstruction A / B name, last_is_ref alternating with the
    layer; the layer-0 access units alone decode to the layer-0 reconstructions"""
    pics = tl.expected(c)
    for k, ((planes, is_ref), p) in enumerate(zip(_decode_all([p.au for p in pics]), pics)):
        assert is_ref == (p.layer == 0), "%s picture %d" % (c.name, k)
        for q in range(3):
            assert np.array_equal(planes[q], p.stages.recon(q)), "%s picture %d plane %d" % (c.name, k, q)
    base = [p for p in pics if p.layer == 0]
    for k, ((planes, is_ref), p) in enumerate(zip(_decode_all([p.au for p in base]), base)):
        assert is_ref
        for q in range(3):
            assert np.array_equal(planes[q], p.stages.recon(q)), "%s base-layer picture %d plane %d" % (c.name, k, q)
    assert sum(p.layer for p in pics) >= 2


@pytest.mark.parametrize("c", tl.CASES, ids=IDS)
def test_sequence_and_headers_of_the_composed_stream(c):
    """the composed access units carry what the sequence rule says: NAL header bytes, frame_num, the override count, no marking
    syntax in a layer-1 slice - read back with the bit reader and held against slice_header_bits()"""
    seq, pics = tl.seq_of(c), tl.expected(c)
    nrefs, idr_id = max(c.refs, 1), 0
    for i, (s, p) in enumerate(zip(seq, pics)):
        assert (s.idr, s.layer) == (p.idr, p.layer)
        slices = [n for n in tl.nal_units(p.au) if n[0] & 0x1F in (1, 5)]
        assert all(n[0] == s.nal_hdr for n in slices), "%s picture %d" % (c.name, i)
        for n in slices:
            r = tl.Bits(tl.unescape(n[1:])[:16])
            r.ue()
            pcm = bool((p.stages.mbinfo()["type"] == tl.MB_IPCM).any())
            want = tl.slice_header_bits(s.idr, s.layer == 1, s.frame_num, idr_id, s.nref, nrefs, tl.qp_of(c, i), pcm or not c.deblock, len(slices))
            assert r.b[r.p:r.p + len(want)] == want, "%s picture %d: slice header" % (c.name, i)
        idr_id = (idr_id + 1) & 0xFF if s.idr else idr_id


def test_what_the_case_list_holds():
    mbs = lambda c: ((c.w + 15) // 16) * ((c.h + 15) // 16)
    assert min(mbs(c) for c in tl.CASES) == 1 and max((c.w, c.h) for c in tl.CASES) == (208, 160) and max(c.pictures for c in tl.CASES) <= 12
    # in every seeded-search case: macroblocks whose layer-1 vector differs from the vector the preceding layer-0 picture left
    for c in tl.SEEDED:
        n = 0
        for p in tl.expected(c):
            if p.layer == 1:
                mb = p.stages.mbinfo()
                inter = np.isin(mb["type"], (1, 5, 6, 7))
                n += int((inter & ((mb["mvx"] != p.prev_mv[0]) | (mb["mvy"] != p.prev_mv[1]))).sum())
        assert n > 0, "%s: wrong motion state would go unnoticed" % c.name
    # a GOP of odd length, and an IDR picture forced behind a layer-1 picture
    odd = tl.BY_NAME["odd_gop_96x80_high"]
    seq = tl.seq_of(odd)
    assert odd.gop & 1 and [i for i, s in enumerate(seq) if s.idr] == [0, 7, 9] and seq[8].layer == 1 and seq[6].layer == 0
    # refs 3: reference counts 1, 2 and 3 in both layers
    r3 = tl.seq_of(tl.BY_NAME["refs3_112x64_main"])
    assert {s.nref for s in r3 if s.layer == 1} == {1, 2, 3} and {s.nref for s in r3 if s.layer == 0 and not s.idr} == {1, 2, 3}
    # 2 and 4 slices
    counts = {len(tl.nal_units(tl.expected(c)[1].au)) for c in tl.CASES}
    assert {1, 2, 4} <= counts
    facts = [(c.name, f) for c in tl.CASES for p in tl.expected(c) if p.layer == 1 for f in p.rewritten.slices]
    # both branches of X; I_PCM behind ordinary macroblocks in one slice; emulation prevention in a rewritten slice; a length that differs
    assert any(f[0] == "plain" for _, f in facts) and any(f[0] == "pcm" for _, f in facts)
    assert any(f[4] for _, f in facts), "no slice holds I_PCM macroblocks behind ordinary ones"
    assert any(f[3] > 0 for _, f in facts), "no rewritten slice needs emulation prevention"
    assert any(f[1] - f[2] == 1 for _, f in facts), "no slice is one byte shorter than the oracle's"
    noise = tl.expected(tl.BY_NAME["noise_48x32"])
    assert all((p.stages.mbinfo()["type"] == tl.MB_IPCM).all() for p in noise if p.layer == 1), "noise: every layer-1 macroblock is I_PCM"
    print("rewritten slices: %d plain, %d with I_PCM, %d one byte shorter, %d emulation prevention bytes" % (
        sum(f[0] == "plain" for _, f in facts), sum(f[0] == "pcm" for _, f in facts), sum(f[1] - f[2] == 1 for _, f in facts), sum(f[3] for _, f in facts)))


@pytest.mark.parametrize("c", tl.CASES, ids=IDS)
def test_base_layer_of_the_composed_stream(c):
    """media_amd.temporal.base_layer / layers on the composed stream: exactly the layer-0 access units"""
    pics = tl.expected(c)
    whole = b"".join(p.au for p in pics)
    want0, want1 = b"".join(p.au for p in pics if p.layer == 0), b"".join(p.au for p in pics if p.layer == 1)
    assert mt.base_layer(whole) == want0
    assert mt.layers(whole) == (want0, want1)
    assert mt.base_layer(want0) == want0 and mt.base_layer(want1) == b""
