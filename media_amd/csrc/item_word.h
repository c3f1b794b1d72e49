// media_amd/csrc/item_word.h -- one picture of a lockstep step as the host knows it (ItemPic, made by PicSeq::pic of
// host_framing.h) and the two device words that carry its facts to the kernels: the position's itemtab word of an indirect launch
// and FrameParams::me of a direct one.  The one place that knows the bit positions.  No HIP: a host compiler builds it alone.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define ITEM_WORD_FN __host__ __device__ __forceinline__
#else
#define ITEM_WORD_FN inline
#endif

namespace {

// item: the batch item (stream) the picture belongs to; cur: the ring slot it is reconstructed into; nref: PicSeq::avail_refs;
// layer, me: PicSeq::layer, me_facts; rband: PicSeq::refresh_band (-1: none)
struct ItemPic { int item, cur, qp, frame_num, idr_id, nref, layer, me, rband; };

// Temporal layers, the two wave-uniform facts k_me takes about its picture (PicSeq::me_facts):
//   ME_PARK       a layer-1 picture: the previous-picture vector word it read is kept in pmv, because its own vectors replace it in MbInfo
//   ME_SEED_PARK  a layer-0 P picture of a two-layer stream: the word comes from pmv, where the layer-1 picture in front of it kept
//                 what the previous LAYER-0 picture left
enum { ME_PARK = 1, ME_SEED_PARK = 2 };

// itemtab word: batch item, ring slot of the picture being coded, the reference pictures the position's picture has (1..3 in a P
// step: reference pictures since the stream's IDR, at most config.refs; 0 in an IDR step), ME_PARK / ME_SEED_PARK, QP, and the
// all-intra band k of an intra refresh picture as k + 1 (0: none; only k_me<IND, true> reads it, k_me.h me_refresh_band)
enum { ITEM_ID_SHIFT = 0, ITEM_ID_MASK = 255, ITEM_CUR_SHIFT = 8, ITEM_CUR_MASK = 3, ITEM_NREF_SHIFT = 10, ITEM_NREF_MASK = 3,
       ITEM_ME_SHIFT = 12, ITEM_ME_MASK = 3, ITEM_QP_SHIFT = 16, ITEM_QP_MASK = 63, ITEM_RFR_SHIFT = 22, RFR_MASK = 63 };
// FrameParams::me of a direct launch: the two facts in bits 0..1, band + 1 in bits 8..13 (launches of k_me<false, true> only)
enum { ME_FACTS_MASK = 3, ME_RFR_SHIFT = 8 };

struct ItemRef { int item, cur, nref, qp, me, rband; };

// the itemtab word of a picture; a field that does not fit its width: 0, and *bad is set
ITEM_WORD_FN uint32_t item_word(const ItemPic& p, bool* bad)
{
    if ((unsigned)p.item > ITEM_ID_MASK || (unsigned)p.cur > ITEM_CUR_MASK || (unsigned)p.nref > ITEM_NREF_MASK || (unsigned)p.me > ITEM_ME_MASK ||
        (unsigned)p.qp > ITEM_QP_MASK || (unsigned)(p.rband + 1) > RFR_MASK) { *bad = true; return 0; }
    return ((uint32_t)p.item << ITEM_ID_SHIFT) | ((uint32_t)p.cur << ITEM_CUR_SHIFT) | ((uint32_t)p.nref << ITEM_NREF_SHIFT) | ((uint32_t)p.me << ITEM_ME_SHIFT) |
           ((uint32_t)p.qp << ITEM_QP_SHIFT) | ((uint32_t)(p.rband + 1) << ITEM_RFR_SHIFT);
}
// FrameParams::me of the picture (refresh: the engine launches the refresh form of k_me, which reads the band)
ITEM_WORD_FN int me_word(const ItemPic& p, bool refresh) { return refresh ? p.me | (int)((unsigned)(p.rband + 1) << ME_RFR_SHIFT) : p.me; }
ITEM_WORD_FN ItemRef item_unpack(uint32_t w)
{
    return ItemRef{(int)((w >> ITEM_ID_SHIFT) & ITEM_ID_MASK), (int)((w >> ITEM_CUR_SHIFT) & ITEM_CUR_MASK), (int)((w >> ITEM_NREF_SHIFT) & ITEM_NREF_MASK),
                   (int)((w >> ITEM_QP_SHIFT) & ITEM_QP_MASK), (int)((w >> ITEM_ME_SHIFT) & ITEM_ME_MASK), (int)((w >> ITEM_RFR_SHIFT) & RFR_MASK) - 1};
}

}  // namespace
