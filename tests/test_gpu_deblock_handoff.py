"""The loop filter on P steps (media_amd/csrc/k_deblock.h, k_deblock_rows_p / k_deblock_pairs_p): ONE launch takes every picture
of the step in the form it needs - with the bS 4 filter when the picture holds intra macroblocks, without it otherwise - and a
row asks again for a hand-off granule that came stale at the top of its iteration, before the vertical edges.  The choice per
picture can only go wrong where one step holds both kinds of picture, so the batches here are mixed: pan + noise items (no
intra macroblock in their P pictures) beside items with a cut or with noise (intra macroblocks), asserted of the oracle
alone before any GPU result is looked at.  Beside that: a picture without any boundary strength, pictures with I_PCM
macroblocks (not filtered at all), pictures of 2 and 3 slices (row form), and the hand-off with one picture in flight and with
thirty-two.  Every case in both forms, compared with the oracle as tests/test_gpu_deblock_lag.py does: every access unit byte for
byte, the reconstruction after the filter sample for sample (in a batch: the first item's last picture; the earlier pictures
are the references of those that follow, so the streams cover them - which is why each mixed batch runs in two orders, once
with an intra item first and once with a plain one).  A filter wait that timed out fails the call (the engine turns
*R.err into an error), so a call that returns is a call whose waits all ended."""
import functools
import numpy as np
import pytest
from media_amd import capi, synth
from oracle_lib import OracleEncoder

gpu = pytest.mark.gpu
FORMS = ["pairs", "rows"]
GOP = 4
MIXED_SIZES = [(64, 48), (176, 144), (16, 64), (64, 16)]
INTRA_TYPES = (0, 3, 4)   # MbInfo type: Intra16x16, I_PCM, Intra4x4


def _pcm_frame(w, h, index, whole):
    """pan + noise with the first macroblock of the second macroblock row - or the whole picture - replaced by uniform noise: at
    the lowest QPs CAVLC would pass 3200 bits there, so the macroblock is I_PCM"""
    if whole:
        return synth.frame_s3(w, h, index)
    f = synth.frame_s1(w, h, index).copy()
    n = synth.frame_s3(w, h, index)
    y, ny = f[:w * h].reshape(h, w), n[:w * h].reshape(h, w)
    y[16:32, 0:16] = ny[16:32, 0:16]
    return f


def _item(kind, w, h, gop, g):
    """the gop pictures of batch item g"""
    if kind == "s1":
        return synth.sequence("s1", w, h, gop, start=5 * g)   # every plain item its own stretch of the pan
    if kind in ("cut", "s3", "s2"):
        return synth.sequence(kind, w, h, gop, start=0 if kind != "s3" else g)
    if kind in ("pcm1", "pcmall"):
        return [_pcm_frame(w, h, g + i, kind == "pcmall") for i in range(gop)]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _oracle(kinds, w, h, qp, gop, slices=0):
    """kinds: one content name per batch item.  (frames, per picture (access unit, (Y, U, V), intra macroblocks, I_PCM
    macroblocks, filter changed a sample)); computed once per configuration and shared, never modified"""
    frames = [f for g, k in enumerate(kinds) for f in _item(k, w, h, gop, g)]
    orc = OracleEncoder(w, h, qp=qp, gop=gop, slices=slices)
    out = []
    for f in frames:
        au = orc.encode(f)[0]
        planes = tuple(orc.recon(p).copy() for p in range(3))
        for a in planes:
            a.setflags(write=False)
        t = orc.mbinfo()["type"]
        changed = any(not np.array_equal(planes[p], orc.recon_pre(p)) for p in range(3))
        out.append((au, planes, int(np.isin(t, INTRA_TYPES).sum()), int((t == 3).sum()), changed))
    orc.close()
    return frames, out


def _steps(kinds, out, gop):
    """per P step i of the batch: ([intra macroblocks of item g's picture i], [filter changed it])"""
    return {i: ([out[g * gop + i][2] for g in range(len(kinds))], [out[g * gop + i][4] for g in range(len(kinds))]) for i in range(1, gop)}


def _mixed_kinds(first):
    """sixteen items: half pan + noise, a quarter with a cut, a quarter noise; `first` puts an intra or a plain item in front"""
    k = ("cut", "s1", "s3", "s1") * 4
    return k if first == "intra" else k[1:] + k[:1]


def _assert_mixed(kinds, w, h, qp, slices=0):
    """the batch proves something only if a P step holds filtered pictures with intra macroblocks beside filtered pictures
    without any"""
    _, out = _oracle(kinds, w, h, qp, GOP, slices)
    mixed = 0
    for i, (intra, changed) in _steps(kinds, out, GOP).items():
        with_i = sum(1 for n, c in zip(intra, changed) if n and c)
        without = sum(1 for n, c in zip(intra, changed) if not n and c)
        print("%dx%d slices %d step %d: %d filtered pictures with intra macroblocks, %d without" % (w, h, slices, i, with_i, without))
        mixed += bool(with_i and without)
    assert mixed, "no P step of this batch holds pictures with and without intra macroblocks"


def _set_form(monkeypatch, form):
    monkeypatch.setenv("MI355X_H264_PAIR_FILTER", "1" if form == "pairs" else "0")


def _single(kinds, w, h, qp, gop, slices=0):
    """item after item through one encoder, one picture in flight; planes compared after every picture"""
    frames, want = _oracle(kinds, w, h, qp, gop, slices)
    enc = capi.Encoder(w, h, qp=qp, gop=gop, slices=slices)
    try:
        for i, f in enumerate(frames):
            assert enc.encode(f)[0] == want[i][0], "picture %d: access unit" % i
            for p in range(3):
                bad = np.argwhere(enc.debug_read(capi.DBG_RECON_Y + p) != want[i][1][p])
                assert bad.size == 0, "picture %d plane %d: first differing sample (row, column) %s" % (i, p, bad[0])
    finally:
        enc.close()


def _batch(kinds, w, h, qp, gop, slices=0):
    import torch
    frames, want = _oracle(kinds, w, h, qp, gop, slices)
    n, fbytes = len(kinds), w * h * 3 // 2
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(w, h, qp=qp, gop=gop, slices=slices, batch=n)
    try:
        cap = 4 * gop * fbytes + 4096
        out, szs, gb = np.zeros(n * cap, np.uint8), np.zeros(n * gop, np.uint32), np.zeros(n, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, out, cap, szs, gb)   # raises on a filter timeout
        for g in range(n):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(w_[0] for w_ in want[g * gop:(g + 1) * gop]), "item %d (%s)" % (g, kinds[g])
        for p in range(3):
            bad = np.argwhere(enc.debug_read(capi.DBG_RECON_Y + p) != want[gop - 1][1][p])
            assert bad.size == 0, "item 0 plane %d: first differing sample (row, column) %s" % (p, bad[0])
    finally:
        enc.close()


# ---- what the GPU cases rely on, stated of the oracle alone (no GPU needed)

@pytest.mark.parametrize("first", ["intra", "plain"])
@pytest.mark.parametrize("w,h", MIXED_SIZES, ids=["%dx%d" % s for s in MIXED_SIZES])
def test_oracle_mixed_batches_hold_both_kinds_of_p_picture(w, h, first):
    _assert_mixed(_mixed_kinds(first), w, h, 33)


@pytest.mark.parametrize("w,h,slices", [(48, 96, 3), (32, 80, 2)])
def test_oracle_sliced_batches_hold_both_kinds_of_p_picture(w, h, slices):
    _assert_mixed(_mixed_kinds("intra"), w, h, 33, slices)


def test_oracle_static_picture_has_no_strength_and_pcm_pictures_are_not_filtered():
    _, out = _oracle(("s2",), 64, 48, 33, GOP)
    assert out[0][4], "the IDR picture is filtered"
    assert any(not changed and not intra for _, _, intra, _, changed in out[2:]), "a static P picture: all P_Skip, nothing to filter"
    for kinds in (("pcm1",), ("pcmall",), ("pcm1", "s1") * 8):
        _, out = _oracle(kinds, 64, 48, 10, GOP)
        nmb = (64 // 16) * (48 // 16)
        for g, k in enumerate(kinds):
            for i in range(GOP):
                _, _, _, pcm, changed = out[g * GOP + i]
                if k == "s1":
                    assert pcm == 0
                else:
                    assert (pcm == nmb) if k == "pcmall" else (0 < pcm < nmb), "item %d picture %d: %d I_PCM macroblocks" % (g, i, pcm)
                    assert not changed, "a picture with an I_PCM macroblock is not filtered"


def test_oracle_handoff_content_is_filtered_with_and_without_intra():
    _, out = _oracle(("cut",), 176, 144, 33, 6)
    assert all(o[4] for o in out) and out[1][2] == 0 and out[2][2] > 0


# ---- the GPU cases

@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("first", ["intra", "plain"])
@pytest.mark.parametrize("w,h", MIXED_SIZES, ids=["%dx%d" % s for s in MIXED_SIZES])
def test_mixed_batch_of_sixteen(monkeypatch, w, h, first, form):
    kinds = _mixed_kinds(first)
    _assert_mixed(kinds, w, h, 33)
    _set_form(monkeypatch, form)
    _batch(kinds, w, h, 33, GOP)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_static_picture_without_any_strength(monkeypatch, form):
    _set_form(monkeypatch, form)
    _single(("s2",), 64, 48, 33, GOP)
    _batch(("s2", "s1") * 8, 64, 48, 33, GOP)   # (beside pictures that are filtered)
    _batch(("s2",) * 16, 64, 48, 33, GOP)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_pictures_with_i_pcm_macroblocks_are_not_filtered(monkeypatch, form):
    _set_form(monkeypatch, form)
    _single(("pcm1",), 64, 48, 10, GOP)
    _single(("pcmall",), 64, 48, 10, GOP)
    _batch(("pcm1", "s1") * 8, 64, 48, 10, GOP)


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w,h,slices", [(48, 96, 3), (32, 80, 2)])
def test_slices(monkeypatch, w, h, slices, form):
    """the pair form is off on pictures of several slices: whatever is asked for, the row form takes the one-launch path"""
    kinds = _mixed_kinds("intra")
    _assert_mixed(kinds, w, h, 33, slices)
    _set_form(monkeypatch, form)
    _single(kinds[:2], w, h, 33, GOP, slices)
    _batch(kinds, w, h, 33, GOP, slices)


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 32])
def test_handoff_one_picture_and_thirty_two(monkeypatch, n, form):
    """176x144 over six pictures: alone, a row's waves start together and the rows wait for one another at every macroblock;
    thirty-two pictures at a time place their waves over time, and rows find granules both published and not yet there"""
    _set_form(monkeypatch, form)
    if n == 1:
        _single(("cut",), 176, 144, 33, 6)
    _batch(("cut", "s1", "s3", "s1") * (n // 4) if n > 1 else ("cut",), 176, 144, 33, 6)
