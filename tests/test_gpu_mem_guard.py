"""Where the kernels write, and what they read before anyone has written it - run with -m gpu on an MI355X.

Every device and pinned block of the library passes one place (media_amd/csrc/dev_mem.h).  With the guard mode on
(mi355x_h264_debug_mem_guard: 262144 bytes of pattern before and behind every block, 0xCB in every block that is not zeroed by
design), the existing small case lists run exactly as their own modules run them - their runners and their comparisons with the
oracle or the independent decoder are imported, not copied - and then every owner's guards, and the zeroed slack behind every
slot of the reconstruction ring, must be untouched, at every check and when the blocks are freed.  A result that depends on what
fresh memory happens to hold differs from the oracle's under poison and fails the imported comparison.

tests/mem_guard.py states the guard size's reasoning, the floors and what is NOT claimed (a store that misses by a whole item
or plane stride; any read out of bounds).  Nothing here provokes a fault: the guards lie inside the library's own allocations and
the biting test's poke is a host-side one-byte hipMemset into them."""
import numpy as np
import pytest

import dec_output as do
import large_batch as lb
import mem_guard as mg
import range_ends as R
import stream_matrix as sm
import test_gpu_dec_group as tdg
import test_gpu_dec_output as tdo
import test_gpu_dec_store as tds
import test_gpu_entropy_random as ter
import test_gpu_large_batch as tlb
import test_gpu_me_zero_gates as tzg
import test_gpu_range_ends as tre
import test_gpu_ref_mix as trm
import test_gpu_rgba_cube as trc
import test_gpu_stream_matrix as tsm
import test_gpu_stream_refs as tsr
from media_amd import capi, h264dec
from oracle_lib import OracleEncoder
from test_entropy_random_oracle import CASES as ENTROPY_CASES
from test_gpu_parity import _compare_all, _padded_planes, _to_nv12
from test_gpu_stream_matrix import tick   # noqa: F401  (the fixture: tools/stream_tick.cpp, built once per module)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- encoder, direct path

@pytest.mark.parametrize("case", mg.direct_cases(), ids=lambda c: c[0])
def test_encoder_direct_path(case):
    """1 IDR + 3 P pictures, every stage against the oracle (test_gpu_parity._compare_all), keep_pre and the quality report on"""
    import torch
    name, kind, w, h, qp, prof, search, slices, refs, door = case
    frames = mg.direct_frames(kind, w, h)
    with mg.guarded() as seen:
        enc = capi.Encoder(w, h, qp=qp, gop=30, profile_idc=prof, slices=slices, refs=refs, search=search, input_format=int(door == "nv12_device"))
        orc = OracleEncoder(w, h, qp=qp, gop=30, profile_idc=prof, slices=slices, refs=refs, search=search)
        try:
            enc.keep_pre(True)
            enc.quality_enable(True)
            for i, f in enumerate(frames):
                if door == "host_padded":
                    au, ft = enc.encode(*_padded_planes(f, w, h, (w + 7, w // 2 + 3, w // 2 + 16), seed=i))
                else:   # NV12 read in place from an odd device address
                    buf = torch.zeros(w * h * 3 // 2 + 1, dtype=torch.uint8, device="cuda")
                    buf[1:] = torch.from_numpy(_to_nv12(np.asarray(f, np.uint8), w, h)).cuda()
                    torch.cuda.synchronize()
                    assert (buf.data_ptr() + 1) % 2 == 1
                    au, ft = enc.encode_device(buf.data_ptr() + 1)
                want, idr = orc.encode(f)
                tag = "%s picture %d" % (name, i)
                assert (ft == capi.FRAME_IDR) == idr == (i == 0), tag
                assert au == want, tag + ": access unit differs from the oracle's"
                _compare_all(enc, orc, tag)
                q = enc.quality()
                assert len(q) == 1 and q[0]["valid"] and q[0]["sse"][0] == mg.luma_sse(orc.recon(0), f, w, h), tag + ": quality record"
        finally:
            enc.close()
            orc.close()
    mg.clean(seen, kinds=["encoder"])
    assert seen[0][2] >= mg.FLOOR["encoder"] + 2 * 6   # the quality report's six pinned blocks were there and guarded


# ---------------------------------------------------------------- lockstep

@pytest.mark.parametrize("kind,search", [("pan", 1), ("scroll", 0)])
def test_lockstep_batch_of_four(kind, search):
    """encode_gops_device with G = 4 at 128x96 (test_gpu_me_zero_gates: both window-load paths of k_me)"""
    with mg.guarded() as seen:
        tzg.test_lockstep_batch_of_four(kind, search)
    mg.clean(seen, kinds=["encoder"])


@pytest.mark.parametrize("name", ["baseline_64", "slices_32"])
def test_large_lockstep_steps(name):
    """64 items (the walk 24 + 24 + 16) and 32 items of three slices (large_batch.run_direct, stages of item 0 after every call)"""
    with mg.guarded() as seen:
        tlb._direct(lb.by_name(name))
    mg.clean(seen, kinds=["encoder"])


# ---------------------------------------------------------------- RGBA ingest

@pytest.mark.parametrize("w,h", [(18, 16), (50, 34)])
def test_rgba_edge_pictures_through_the_engine(w, h):
    """value_cube's edge pictures (w % 4 == 2) through k_rgba_to_i420 from tight and padded host rows and from device memory"""
    with mg.guarded() as seen:
        trc.test_edge_pictures_through_the_encoder(w, h)
    mg.clean(seen, kinds=["encoder"])
    assert seen[0][2] >= mg.FLOOR["encoder"] + 2 * 2   # the RGBA staging pair came with the first host picture


# ---------------------------------------------------------------- slice bands

def test_two_band_instances_with_halo_exchange():
    """two band instances of one picture, three reference pictures, halo rows exported and imported (test_gpu_ref_mix)"""
    with mg.guarded() as seen:
        trm.test_band_instances_read_the_older_pictures_halo_rows("fast_96x128", 2)
    mg.clean(seen, checks=2, kinds=["encoder"])


# ---------------------------------------------------------------- entropy stage alone

@pytest.mark.parametrize("c", [ENTROPY_CASES[1], ENTROPY_CASES[0]], ids=["dense_16x16", "encoder_shaped_16x16"])
def test_injected_syntax(c):
    """the dense and the encoder-shaped case of test_gpu_entropy_random at their smallest size"""
    with mg.guarded() as seen:
        ter.test_injected_syntax_codes_to_the_oracles_bytes(c)
    mg.clean(seen, kinds=["encoder"])
    assert seen[0][2] >= mg.FLOOR["encoder"] + 2   # d_inject_src


@pytest.mark.parametrize("batch", [1, 2])
def test_refused_slice_writes_nothing_past_a_buffer(batch):
    """MI355X_H264_E_OVERFLOW: "nothing is written past the buffer" - the guards behind S.d_bitbuf, S.h_au, d_slotcode and
    d_slotbits are the proof"""
    with mg.guarded() as seen:
        ter.test_first_slice_over_its_share_is_refused_and_nothing_else_is_touched(batch)
    mg.clean(seen, kinds=["encoder"])


# ---------------------------------------------------------------- stream hub

@pytest.mark.parametrize("c", range(len(mg.DIRECT_SIZES)), ids=["%dx%d" % s for s in mg.DIRECT_SIZES])
def test_hub_geometry_groups(tick, monkeypatch, c):   # noqa: F811
    """the geometry groups of the fixed sizes, three streams each, as test_gpu_stream_matrix.test_geometry_sweep runs them"""
    group = sm.geometry()[c]
    assert (group[0].w, group[0].h) == mg.DIRECT_SIZES[c]
    with mg.guarded() as seen:
        tsm.steps_of(tsm.run_group(tick, monkeypatch, group, ctx=1))
    mg.clean(seen, kinds=["stream"])


def test_hub_churn(tick, monkeypatch):   # noqa: F811
    with mg.guarded() as seen:
        tsm.test_forced_idr_and_stream_churn_under_load(tick, monkeypatch)
    mg.clean(seen, kinds=["stream"])


def test_hub_six_streams_of_one_two_and_three_usable_references(tick, monkeypatch):   # noqa: F811
    with mg.guarded() as seen:
        tsr.test_mixed_counts_in_one_step(tick, monkeypatch)
    mg.clean(seen, kinds=["stream"])


def test_hub_rgba_group_of_three_streams():
    """k_rgba_to_i420_step at 18x16"""
    with mg.guarded() as seen:
        trc.test_edge_pictures_through_three_streams_of_one_engine(18, 16)
    mg.clean(seen, kinds=["stream"])
    assert seen[0][2] >= mg.FLOOR["stream"] + 2 * 2   # the hub's RGBA staging pair


# ---------------------------------------------------------------- decoder

@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_decoder_at_the_range_ends(case):
    with mg.guarded() as seen:
        tre.test_decoder_equals_the_independent_decoder_at_the_range_ends(case)
    mg.clean(seen, kinds=["decoder"])


def test_decoder_group_whose_lists_of_large_levels_grow():
    """four streams; the lists grow twice: blocks are dropped and made again under guard (the tally), k_dec_patch writes through them"""
    with mg.guarded() as seen:
        tre.test_group_of_four_streams_and_the_growth_of_the_lists_of_large_levels()
    mg.clean(seen, kinds=["group"])


def test_decoder_group_sit_out_schedule_and_a_truncated_unit():
    with mg.guarded() as seen:
        tdg.test_streams_that_sit_out_and_empty_units()
        tdg.test_a_failing_stream_fails_alone()
    mg.clean(seen, checks=2, kinds=["group"])


def test_decoder_resize_up_and_down():
    """64x48, 96x80 and 64x48 again through one Decoder: every change of the coded size frees the store and the arrays (checked as
    they go: the tally) and makes them again under guard; pictures and budget as test_gpu_dec_store has them"""
    import dec_group as dg
    small, big = dg.stream_pictures(dg.BY_NAME["five_64x48"], 0), dg.stream_pictures(dg.BY_NAME["one_96x80"], 0)
    with mg.guarded() as seen:
        dec = h264dec.Decoder()
        try:
            for tag, (au, planes, i420, size), (w, h) in (("64x48", small[0], (64, 48)), ("96x80", big[0], (96, 80)), ("64x48 again", small[0], (64, 48))):
                assert dec.decode(au), tag
                for p in range(3):
                    assert np.array_equal(dec.plane(p), planes[p]), "%s plane %d" % (tag, p)
                assert dec.info()[:2] == size and np.array_equal(dec.i420(), i420), tag
                tds.within(dec.last_step(), tds.budget(w, h, 1), tag)   # the caller's bytes: guards are not counted
                assert dec.mem_check()[0] == 0, tag
        finally:
            dec.close()
    mg.clean(seen, kinds=["decoder"])


# ---------------------------------------------------------------- decoder output

@pytest.mark.parametrize("name", ["out_50x34", "out_18x18"])
def test_decoder_output_read_all(name):
    """all four layouts at the cropped sizes 14x16, 18x18, 46x30 and 50x34, row_align 1 / 64 / 256, to host and to device; the
    destination's 0xA5 comparison is the imported test's own"""
    with mg.guarded() as seen:
        tdo.test_read_all_to_host_and_device(do.BY_NAME[name])
    mg.clean(seen, kinds=["group"])


def test_decoder_output_armed_group_and_single_read():
    with mg.guarded() as seen:
        tdo.test_armed_output_follows_every_step("out_50x34")
        tdo.test_single_decoder_read_equals_the_groups()
    mg.clean(seen, checks=2, kinds=["group"])


# ---------------------------------------------------------------- the guards bite; the default is off

def _lines(lines):
    return sorted(lines[1:])


def test_the_check_reports_a_poked_byte_with_name_side_and_offset():
    g, w, h = mg.GUARD, 48, 32
    frames = mg.direct_frames("s1", w, h, 2)
    with mg.guarded() as seen:
        enc = capi.Encoder(w, h, qp=30)
        grp = h264dec.DecoderGroup(2)
        try:
            aus = [enc.encode(f)[0] for f in frames]
            for au in aus:
                assert [got for _, got in grp.decode([au, au])] == [1, 1]
            # the LAST block: the encoder's is the third slot's S.h_au (st_au bytes: a multiple of 256 above twice the picture plus
            # 64 KiB, which the test does not restate - it walks to the one offset that is accepted after a refused one), the
            # group's its device list of large levels (1024 entries of 8 bytes)
            for owner, pinned, last, sizes in ((enc, "h_stage", "S.h_au", range(256, 1 << 20, 256)), (grp, "h_tab[k]", "d_big", (1024 * 8,))):
                assert owner.mem_check()[0] == 0
                blocks, slack = mg.header(owner.mem_check()[2])
                assert owner.mem_poke("#0", -1, 0) == 0                 # the last byte of the guard before the first block
                n = next(n for n in sizes if owner.mem_poke("#-1", n - 1, 0) == capi.E_ARG and owner.mem_poke("#-1", n, 0) == 0)
                assert owner.mem_poke(pinned, -g // 2, 0) == 0          # the middle of a pinned block's guard
                assert owner.mem_poke("#-1", -g - 1, 0) == capi.E_ARG and owner.mem_poke("#-1", n + g, 0) == capi.E_ARG   # beyond the guards
                damaged, regions, lines = owner.mem_check()
                assert damaged == 3 and regions == 2 * blocks + slack, lines
                assert _lines(lines) == sorted(["d_plane_base[0] before first=-1 last=-1 bytes=1",
                                                "%s after first=%d last=%d bytes=1" % (last, n, n),
                                                "%s before first=%d last=%d bytes=1" % (pinned, -g // 2, -g // 2)]), lines
                for off in (0, 1, 15):                                   # the caller's bytes are refused
                    assert owner.mem_poke("d_plane_base[0]", off, 0) == capi.E_ARG
                    assert owner.mem_poke(pinned, off, 0) == capi.E_ARG
                assert owner.mem_poke("no_such_block", -1, 0) == capi.E_ARG and owner.mem_poke("#%d" % blocks, -1, 0) == capi.E_ARG
                assert owner.mem_poke("#0", -1, -1) == 0 and owner.mem_poke(pinned, -g // 2, -1) == 0 and owner.mem_poke("#-1", n, -1) == 0   # put back
                assert owner.mem_check()[0] == 0
        finally:
            enc.close()
            grp.close()
    mg.clean(seen, checks=2, kinds=["encoder", "group"])


def test_the_default_is_off():
    """an owner created without the switch holds the bytes it always did (test_gpu_dec_store's budget) and answers the check
    with MI355X_H264_E_ARG: "never guarded" is not "intact" """
    was = capi.mem_guard(0)
    try:
        assert capi.mem_guard_get() == (0, False)
        tds.test_a_group_holds_its_store_and_its_sets_and_does_not_grow()
        enc, dec, grp = capi.Encoder(32, 32), h264dec.Decoder(0), h264dec.DecoderGroup(2)
        st = capi.Stream(32, 32)
        try:
            au = enc.encode(mg.direct_frames("s1", 32, 32, 1)[0])[0]
            assert dec.decode(au) and grp.decode([au, None])[0] == (0, 1)
            st.encode(mg.direct_frames("s1", 32, 32, 1)[0])
            for owner in (enc, st, dec, grp):
                with pytest.raises(capi.EncoderError) as ei:
                    owner.mem_check()
                assert ei.value.rc == capi.E_ARG and "without guards" in str(ei.value), str(ei.value)
            assert enc.mem_poke("#0", -1, 0) == capi.E_ARG and grp.mem_poke("#0", -1, 0) == capi.E_ARG
            tds.within(grp.last_step(), tds.budget(32, 32, 2), "unguarded group")
        finally:
            for owner in (enc, st, dec, grp):
                owner.close()
    finally:
        capi.mem_guard(*was)
