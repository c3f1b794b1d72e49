/*
 * oracle/h264_oracle.h -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement ("oracle") of the H.264 encode hot path that the reference
 * delegates to ISVCEncoder::EncodeFrame
 * (/root/reference/video_codec/VideoEncoderOpenH264.cpp:344), plus a test-side
 * decoder used for encode->decode round trips.
 *
 * PARITY UNPINNED vs OpenH264: the reference ships no codec source, no
 * libopenh264.so, no tests and no golden vectors.
 * What pins this oracle instead: (i) known answers from ITU-T H.264 held in
 * tests/, (ii) encoder reconstruction == decoder output byte for byte, which
 * ties every normative stage to the standard.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library.  The product (media_amd/) never does.
 */
#ifndef ORACLE_H264_ORACLE_H
#define ORACLE_H264_ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout of one macroblock's quantised levels (int16), shared with the GPU
 * path's debug dump so the two can be compared array-for-array. */
enum {
    H264O_LV_LUMA_DC = 0,     /* 16: Intra16x16 DC levels, zig-zag order            */
    H264O_LV_LUMA = 16,       /* 16 blocks (blkIdx order) x 16 levels, zig-zag      */
    H264O_LV_CHROMA_DC = 272, /* Cb 4, Cr 4 (raster 2x2 order = chroma DC scan)     */
    H264O_LV_CHROMA_AC = 280, /* Cb blk0..3, Cr blk0..3, x16 zig-zag (idx0 unused)  */
    H264O_LV_STRIDE = 416     /* int16 per macroblock (832 B)                       */
};

enum { H264O_MB_I16 = 0, H264O_MB_P16 = 1, H264O_MB_PSKIP = 2, H264O_MB_IPCM = 3, H264O_MB_I4 = 4,
       H264O_MB_P16X8 = 5, H264O_MB_P8X16 = 6, H264O_MB_P8X8 = 7 };   /* 5..7: two 16x8, two 8x16, four 8x8 partitions (one reference) */
#define H264O_MB_IS_INTRA(t) ((t) == H264O_MB_I16 || (t) == H264O_MB_IPCM || (t) == H264O_MB_I4)

typedef struct {
    int32_t width, height;  /* display size, even, 16..4096                          */
    int32_t fps;            /* 30 or 60 (level selection only)                       */
    int32_t qp;             /* fixed frame QP, 10..51                                */
    int32_t gop;            /* IDR period in frames (uiIntraPeriod, ref :242)        */
    int32_t profile_idc;    /* 66 baseline, 77 main (CAVLC), 100 high (no 8x8)       */
    int32_t disable_deblock;/* 0: in-loop filter on (ref :295 iLoopFilterDisableIdc) */
    int32_t slices;         /* 0/1: one slice per picture (the reference preset, SM_SINGLE_SLICE :247); n > 1: n bands of
                             * ceil(rows / n) macroblock rows, one slice NAL each, no loop filtering across them      */
    int32_t band_index;     /* band_count > 1: this instance codes only its share of the slices (slice bands of one   */
    int32_t band_count;     /* picture on several instances / GPUs, mirrors mi355x_h264_config)                       */
    int32_t refs;           /* 0/1: one reference frame (the reference preset, iNumRefFrame = 1 :290); 2, 3: the motion
                             * search runs on the last `refs` pictures (BASELINE.json configs[4]), ref_idx_l0 is coded      */
    int32_t search;         /* integer motion search (mirrors mi355x_h264_config.search): 0 = exhaustive +-16 around the co-located
                             * macroblock; 1 = seeded - when the macroblock's previous-picture vector, rounded to integer samples,
                             * is a strict local minimum of the search cost among its eight integer neighbours, it is taken as
                             * the integer winner and the exhaustive pass is skipped (it runs whenever the test fails)         */
} h264o_config;

typedef struct h264o_enc h264o_enc;
typedef struct h264o_dec h264o_dec;

/* per-macroblock side information exposed for stage-by-stage parity checks */
typedef struct {
    int16_t mvx, mvy;      /* quarter-pel motion vector (0 for intra); with partitions: that of the first one */
    uint8_t type;          /* H264O_MB_*                                            */
    uint8_t i16_mode;      /* Intra16x16PredMode 0..3; inter: transform_size_8x8_flag */
    uint8_t chroma_mode;   /* intra_chroma_pred_mode 0..3; inter: ref_idx_l0          */
    uint8_t cbp;           /* coded_block_pattern (luma | chroma<<4)                */
    uint8_t tc[24];        /* TotalCoeff per 4x4: 16 luma (blkIdx), 4 Cb, 4 Cr      */
} h264o_mbinfo;            /* 32 bytes                                              */

h264o_enc *h264o_enc_create(const h264o_config *cfg);
void h264o_enc_destroy(h264o_enc *e);
/* Encode one I420 picture.  Returns bytes written (Annex B, 4-byte start codes;
 * SPS+PPS precede every IDR) or <0 on error.  *is_idr receives 1 for IDR. */
int64_t h264o_enc_encode(h264o_enc *e, const uint8_t *y, int ys, const uint8_t *u, int us,
                         const uint8_t *v, int vs, int force_idr, uint8_t *out, size_t out_cap,
                         int *is_idr);
/* picture QP for the pictures that follow (mirrors mi355x_h264_set_qp) */
int h264o_enc_set_qp(h264o_enc *e, int qp);
/* idr_pic_id of the next IDR and its increment per IDR (mod 256): lets closed GOPs of one
 * stream be encoded by different instances and still concatenate to the serial stream */
int h264o_enc_set_idr_id(h264o_enc *e, int next, int step);
/* band mode: reference rows next to the band, exchanged with the neighbours (mirrors mi355x_h264_band_halo_*) */
size_t h264o_enc_halo_bytes(const h264o_enc *e);
void h264o_enc_halo_export(h264o_enc *e, int edge, uint8_t *dst);
void h264o_enc_halo_import(h264o_enc *e, int edge, const uint8_t *src);
/* Accessors valid until the next encode call.  Planes are coded size
 * (multiples of 16), pitch == coded width (chroma: half). */
int h264o_enc_coded_width(const h264o_enc *e);
int h264o_enc_coded_height(const h264o_enc *e);
const uint8_t *h264o_enc_recon(const h264o_enc *e, int plane);       /* deblocked */
const uint8_t *h264o_enc_recon_pre(const h264o_enc *e, int plane);   /* before loop filter */
const h264o_mbinfo *h264o_enc_mbinfo(const h264o_enc *e);
/* 8 int16 per macroblock beside mbinfo: the vectors (x, y) of the four 8x8 quadrants of an inter macroblock (a 16x16
 * macroblock carries its vector four times, a 16x8 one twice twice ...) */
const int16_t *h264o_enc_mvq(const h264o_enc *e);
/* 16 bytes per macroblock beside mbinfo: Intra4x4PredMode of the 16 blocks (blkIdx order) for H264O_MB_I4 */
const uint8_t *h264o_enc_mbaux(const h264o_enc *e);
/* Intra4x4 prediction (8.3.1.2) of one block: rec points at the block inside the picture under reconstruction;
 * avail bit0 left, bit1 top, bit2 top-left, bit3 top-right.  Returns 0, or -1 when the mode needs unavailable samples */
int h264o_pred4x4(const uint8_t *rec, int stride, int mode, int avail, uint8_t pred[16]);
const int16_t *h264o_enc_levels(const h264o_enc *e);
/* bits of slice_data() of the last slice, before trailing bits (for tests) */
int64_t h264o_enc_last_slice_bits(const h264o_enc *e);
/* every slice of the last picture: bits of its RBSP from first_mb_in_slice up to and including rbsp_stop_one_bit; returns the
 * number of slices (at most `cap` entries are written) */
int h264o_enc_slice_bits_all(const h264o_enc *e, int64_t *bits, int cap);
/* per macroblock of the last picture: the bit of its slice's RBSP at which its syntax starts (a P_Skip macroblock: where the
 * mb_skip_run that holds it is written) - lets a test name the macroblock a differing byte falls in */
const uint32_t *h264o_enc_mb_bitpos(const h264o_enc *e);
/* source planes (coded size, pitch as the reconstruction's): of the last encoded picture, or the samples
 * h264o_enc_random_picture drew for its I_PCM macroblocks */
const uint8_t *h264o_enc_source(const h264o_enc *e, int plane);
/* What the slice data writer has written since the last reset, per syntax element (tests: is an input worth running?).
 * Counted for h264o_enc_encode and h264o_enc_random_picture alike; every field is a plain count unless named max_. */
typedef struct {
    uint32_t coeff_token[4][17][4];     /* Table 9-5 by [nC class: 0-1, 2-3, 4-7, 8+][TotalCoeff][TrailingOnes] */
    uint32_t cdc_token[5][4];           /* ... its chroma DC column (nC = -1) */
    uint32_t total_zeros[16][16];       /* Tables 9-7 / 9-8 by [TotalCoeff 1..15][total_zeros] */
    uint32_t cdc_total_zeros[4][4];     /* Table 9-9 (a) by [TotalCoeff 1..3][total_zeros] */
    uint32_t run_before[8][15];         /* Table 9-10 by [min(zerosLeft, 7)][run_before] */
    uint32_t suffix_len[7];             /* levels coded with suffixLength 0..6 */
    uint32_t prefix14[7], prefix15[7];  /* levels of level_prefix 14 / 15, by the suffixLength they were coded with */
    uint32_t mb_kind[8];                /* by H264O_MB_* */
    uint32_t mb_type[2][32];            /* mb_type as written, [0] in I slices, [1] in P slices */
    uint32_t cbp_intra[48], cbp_inter[48];   /* coded_block_pattern of Intra4x4 / inter macroblocks, by value */
    uint32_t i4_mode[16][9];            /* Intra4x4PredMode by [blkIdx][mode] */
    uint32_t max_mvd;                   /* greatest |mvd_l0| component, quarter samples */
    uint32_t max_skip_run, skip_runs_over_a_row, skip_run_ends_slice, pcm_after_skip_run;
    uint32_t long_header_slots;         /* macroblock headers (mb_type .. mb_qp_delta) of more than 64 bits */
    uint32_t long_residual_slots;       /* residual blocks of more than 64 bits */
    /* picture level, h264o_enc_random_picture with features 16384 / 32768 / 65536 */
    uint32_t nonref_pics;               /* pictures of nal_ref_idc 0 */
    uint32_t nonref_run[4];             /* runs of 1, 2, 3 of them (counted when the next reference picture is written; [0] unused) */
    uint32_t nonref_before_idr, nonref_after_idr;   /* such a picture directly before / directly after an IDR picture */
    uint32_t slice_shape[4];            /* non-IDR pictures: all slices I, an I slice first and a P slice later, a P slice first and an I slice later, all P */
    uint32_t slice_type_form[2];        /* ... with slice_type written as 0..4 / as 5..9 */
    uint32_t pps_switches;              /* pictures that name another PPS than the picture before */
    uint32_t pps_resent;                /* PPS sent again with changed content in front of a non-IDR picture */
    uint32_t pics_no_dbf_ctrl;          /* pictures under a PPS with deblocking_filter_control_present_flag = 0 */
    uint32_t pps_id_used[4];            /* pictures by pic_parameter_set_id 0, 1, 7, 255 */
    uint32_t sps_id_used[3];            /* streams by seq_parameter_set_id 0, 5, 31 */
    uint32_t crop_lt_streams;           /* streams whose SPS crops on the left / top */
    /* h264o_enc_random_picture with feature 131072 ("range ends") */
    uint32_t re_slice_qp[52];           /* slices by SliceQP_Y (pic_init_qp_minus26 + slice_qp_delta as written) */
    uint32_t re_prefix15_max[7];        /* levels of level_prefix 15 whose suffix is all ones, by suffixLength: the largest magnitude it codes */
    uint32_t re_prefix16[3];            /* levels of level_prefix >= 16 in Intra16x16 DC blocks, in chroma DC blocks, anywhere else */
    uint32_t re_mv_limit[4];            /* vectors written at -8192, at 8191 (horizontal), at -2048, at 2047 (vertical), quarter samples */
    uint32_t re_mvd_over_8192;          /* mvd_l0 components of magnitude above 8192 */
    uint32_t re_qpi_below_0, re_qpi_above_51;   /* macroblocks with chroma residual whose QP_Y + chroma_qp_index_offset (either) is < 0 / > 51 */
    uint32_t re_dropped;                /* levels the generator took out again because a bound of 8.5 would not have held */
} h264o_hits;
const h264o_hits *h264o_enc_hits(const h264o_enc *e);
void h264o_enc_hits_reset(h264o_enc *e);
/* scene-change statistic (mirrors mi355x_h264_last_me_cost) */
uint32_t h264o_enc_last_me_cost(const h264o_enc *e);
/* one byte per macroblock of the last P picture (stale after an IDR picture): what the motion stage decided before anything was
 * coded - 0 searched and coded as an inter macroblock, 1 searched and handed to the intra pass, 2 settled without a search by one
 * of the "nothing left to code" tests (mirrors the searched / tq_coded counters of mi355x_h264_stats) */
const uint8_t *h264o_enc_p_decision(const h264o_enc *e);

/* One picture of RANDOM conforming syntax (decoder-peer tests; nothing is reconstructed - oracle/h264_dec.c says what the
 * stream decodes to).  features: 1 mb_qp_delta + slice QPs, 2 chroma_qp_index_offsets, 4 filter offsets, 8 I_PCM macroblocks,
 * 16 a random disable_deblocking_filter_idc, 32 inter macroblocks written from random draws as such: sub_mb_types down to 4x4, a
 * ref_idx_l0 per partition, random mvd_l0 (the vectors are then whatever the decoder adds up: mvq / mbinfo vectors are not filled),
 * 64 (with 32) slices cut at random macroblocks instead of bands of rows, 128 ref_pic_list_modification commands in P slices,
 * 256 parameter sets and slice headers laid out the way OpenH264 writes them (15-bit frame_num, POC type 0, VUI, a list modification
 * in every P slice; the same for every picture of a stream), 512 levels of 128 .. 427 at QP_Y <= 14 (use with 1: QPs are then drawn from 4 .. 48),
 * 1024 constrained_intra_pred_flag = 1,
 * 2048 dense residual: blocks of shapes the quantised transform of a picture hardly ever makes - every position non-zero, one late
 * coefficient after a long run of zeros, runs of +-1 with 0..3 trailing ones in front of a level of exactly +-2 / +-3, magnitude ramps
 * that walk suffixLength from 0 to 6, levels of level_prefix 14 and 15 at every suffixLength, TotalCoeff and TrailingOnes drawn
 * evenly - beside the ordinary ones, within a budget per macroblock (level_prefix stays <= 15),
 * 4096 encoder-shaped: what mi355x_h264_debug_code_syntax turns into the same bytes.  A P_L0_16x16 macroblock that k_mvpred would
 * turn into P_Skip (no coefficients, ref_idx 0, the P_Skip vector) gets its vector moved by a quarter sample; a picture with an
 * I_PCM macroblock says disable_deblocking_filter_idc 1; the I_PCM samples outside the display size repeat the edge (the
 * encoder reads a display-size source); and - what the decision kernels' pictures have and independent draws never do - now and
 * then a run of P_Skip macroblocks longer than a row, and I_PCM samples that are all zero (emulation prevention),
 * 8192 (tests of the refusal path only, NOT conforming: macroblocks far beyond the 3200 bits of A.3.1) two macroblocks in five of
 * the first slice carry escape levels in every position.
 * 16384 non-reference pictures (nal_ref_idc 0, no dec_ref_pic_marking, frame_num = PrevRefFrameNum + 1; one between reference
 * pictures, with 256 - POC type 0 - runs of up to three), 32768 every slice of a non-IDR picture is an I or a P slice (all-I non-IDR
 * pictures, I before P, P before I, all-P; slice_type 7 / 5 only when all slices share the type; one slice per picture: I and P
 * take turns), 65536 parameter sets: seq_parameter_set_id from {0, 5, 31}, two to four PPS with ids from {0, 1, 7, 255}, each
 * with its own pic_init_qp, chroma offsets, num_ref_idx_l0_default_active, deblocking_filter_control_present_flag,
 * constrained_intra_pred_flag and (High) transform_8x8_mode_flag, all sent with the IDR picture, one sent again with new content
 * before some non-IDR pictures, one PPS per picture; and frame cropping on the left and top by 2 or 4 luma samples.
 * 131072 "range ends": the ends of the QP, level and vector ranges.  With 1: slice and macroblock QPs from 0 .. 51, about half of
 * them from {0, 1, 2, 3, 49, 50, 51} (mb_qp_delta in its wrapped form; pic_init_qp 26 and slice_qp_delta -26 .. 25 reach SliceQP_Y
 * 0 and 51).  Vectors are drawn as vectors (with 32: for every partition down to 4x4 and every reference index, predicted by a
 * statement of 8.4.1.3 on the 4x4 grid of the writer's own; mvd_l0 is whatever results): one partition in ten uniform over the
 * range A.3.1 allows at the level_idc written (-8192 .. 8191 by -2048 .. 2047 quarter samples), one in ten exactly at a limit -
 * every second time the limit opposite to the predictor, so |mvd_l0| passes 8192 -, never outside.  Levels: in macroblocks of
 * QP_Y <= 11 some blocks carry one large level - the largest magnitude level_prefix 15 codes at suffixLength 0 .. 6 (2064, 2063,
 * 2078, 2108, 2168, 2288, 2528, negative: the suffix is all ones; the levels in front of it walk suffixLength there), exactly
 * +-127 / +-128 / +-129, and under High in Intra16x16 DC and chroma DC blocks a level of level_prefix 16 (2064 .. 6159 at
 * suffixLength 0; never 17: a quantiser of 8-bit video makes no level above 6528).  Picture 5 of every 12 of a stream is all
 * QP_Y 0 / 1 with one block in three full of +-127 .. +-130, picture 9 with every block of every macroblock (the lists of large levels of
 * a decoder outgrow what they start with, then what they grew to).  Conformance (8.5.10 - 8.5.13): for every block the sum of
 * the magnitudes of its scaled coefficients (DC from the DC transform of the magnitudes; 8x8: weighted 1.5 per odd row / column)
 * bounds every intermediate; while it passes 32000 the largest level of the block is taken out again (h264o_hits.re_dropped).
 * oracle/h264_dec.c measures the intermediates themselves (h264o_dec_stat).
 * 262144 "prediction cells" (with 32): the vector of every partition is drawn per component - one in eight near its predictor, one in
 * eight within +-8 samples, otherwise with a fraction drawn evenly and one end of the window 8.4.2.2.1 reads for it put 0 .. 5 samples
 * inside or 1 .. 8 outside one edge of the picture (either end of the window about either edge) -, and of the macroblocks of a P slice 17 %
 * are Intra16x16, 20 % Intra4x4, 5 % I_PCM, 16 % P_Skip and 18 % P_8x8 (intra prediction modes are drawn evenly over what availability allows
 * anyway); levels are taken out
 * again as under 131072 while a block passes the bound of 8.5.  oracle/h264_dec.c says which cells of its prediction account (h264o_dec_pred) that reaches.
 * These five draw from generators of their own.  2048, 4096 and 8192 draw only when set: streams of every other feature value stay what they were.  mbqp_out (one byte per macroblock, may be NULL) receives QP_Y of every
 * macroblock (0 for I_PCM, the value the loop filter uses).  Side information: h264o_enc_mbinfo / _mvq / _mbaux / _levels. */
int64_t h264o_enc_random_picture(h264o_enc *e, uint32_t seed, int force_idr, int features, uint8_t *out, size_t out_cap,
                                 int *is_idr, uint8_t *mbqp_out);

/* the last picture of h264o_enc_random_picture: is a reference picture, pic_parameter_set_id, seq_parameter_set_id, left crop and
 * top crop in luma samples, pic_init_qp, slice-type shape (h264o_hits.slice_shape; an IDR picture: 0), deblocking control present */
void h264o_enc_random_last(const h264o_enc *e, int32_t out[8]);

/* ---- stand-alone stage functions (kernel-level parity, known-answer tests) ---- */
void h264o_fdct4x4(const int16_t in[16], int16_t out[16]);
void h264o_idct4x4_add(const int16_t coef[16], uint8_t *dst, int stride);
/* quantise one 4x4 of forward-transform output (raster); intra selects the
 * rounding offset; returns levels in raster order */
void h264o_quant4x4(const int16_t w[16], int qp, int intra, int16_t lv[16]);
void h264o_dequant4x4(const int16_t lv[16], int qp, int16_t out[16]);
/* High profile 8x8 transform: forward (non-normative), quantiser, 8.5.13 scaling and inverse transform */
void h264o_fdct8x8(const int16_t in[64], int32_t out[64]);
void h264o_quant8x8(const int32_t w[64], int qp, int intra, int16_t lv[64]);
void h264o_dequant8x8(const int16_t lv[64], int qp, int32_t out[64]);
void h264o_idct8x8_add(const int32_t coef[64], uint8_t *dst, int stride);
/* luma quarter-pel and chroma eighth-pel motion compensation (8.4.2.2) on a
 * w x h plane with edge clamping */
void h264o_mc_luma(const uint8_t *ref, int stride, int w, int h, int x, int y, int mvx, int mvy,
                   int bw, int bh, uint8_t *dst, int dstride);
/* spec-literal one-sample evaluation of 8.4.2.2.1 (cross-check of the block form) */
int h264o_luma_sample_ref(const uint8_t *ref, int stride, int w, int h, int x, int y, int mvx, int mvy);
void h264o_mc_chroma(const uint8_t *ref, int stride, int w, int h, int x, int y, int mvx,
                     int mvy, int bw, int bh, uint8_t *dst, int dstride);
int h264o_sad16x16(const uint8_t *a, int as, const uint8_t *b, int bs);
int h264o_satd16x16(const uint8_t *a, int as, const uint8_t *b, int bs);
int h264o_satd8x8(const uint8_t *a, int as, const uint8_t *b, int bs);
/* (sum over the 4x4 blocks of a w x h rectangle of |Hadamard|) >> 1; w, h multiples of 4 */
int h264o_satd_rect(const uint8_t *a, int as, const uint8_t *b, int bs, int w, int h);
/* intra predictors; avail bit0 = left, bit1 = top, bit2 = top-left */
void h264o_pred16x16(const uint8_t *rec, int stride, int mode, int avail, uint8_t pred[256]);
void h264o_pred_chroma8x8(const uint8_t *rec, int stride, int mode, int avail, uint8_t pred[64]);
/* deblock a whole picture in place given per-MB info (8.7); slice_of (slice index per macroblock) non-NULL =
 * disable_deblocking_filter_idc 2, edges between different slices are left alone; macroblock rows row0..row1-1 */
void h264o_deblock_picture(uint8_t *y, uint8_t *u, uint8_t *v, int cw, int ch,
                           const h264o_mbinfo *mbs, const int16_t *mvq, int qp, const int16_t *slice_of, int row0, int row1);
/* Exp-Golomb / CAVLC helpers for known-answer tests */
/* RGBA ingest (h264_rgba.c): rgba = R, G, B, A bytes per sample, stride in bytes; i420 = w*h*3/2 bytes */
void h264o_rgba_to_i420(const uint8_t *rgba, int stride, int w, int h, uint8_t *i420);
int h264o_ue_bits(uint32_t v, uint32_t *code); /* returns length, *code = bit pattern */
int h264o_se_bits(int32_t v, uint32_t *code);
/* writes one residual block with CAVLC; returns number of bits appended to buf
 * (MSB first, buf must be zeroed, cap >= 64 bytes) */
int h264o_cavlc_block(const int16_t *lv, int max_coeff, int nC, uint8_t *buf);
size_t h264o_nal_escape(const uint8_t *rbsp, size_t n, uint8_t *out);

/* ---- decoder ---- */
h264o_dec *h264o_dec_create(void);
void h264o_dec_destroy(h264o_dec *d);
/* Feed one access unit (any number of Annex B NALs).  Returns 1 when a picture
 * was completed, 0 for parameter sets only, <0 on a syntax/feature error. */
int h264o_dec_decode(h264o_dec *d, const uint8_t *data, size_t len);
int h264o_dec_width(const h264o_dec *d);         /* cropped */
int h264o_dec_height(const h264o_dec *d);
int h264o_dec_crop_left(const h264o_dec *d);     /* frame_crop_left_offset / _top_offset in luma samples: the cropped picture starts there in plane() */
int h264o_dec_crop_top(const h264o_dec *d);
int h264o_dec_last_is_ref(const h264o_dec *d);   /* the last picture had nal_ref_idc != 0 */
int h264o_dec_ref_age(const h264o_dec *d, int idx);   /* RefPicList0[idx] of its last P slice: reference pictures decoded since that one (-1 none) */
int h264o_dec_coded_width(const h264o_dec *d);
int h264o_dec_coded_height(const h264o_dec *d);
const uint8_t *h264o_dec_plane(const h264o_dec *d, int plane); /* coded size, pitch = coded w */
const char *h264o_dec_error(const h264o_dec *d);
int h264o_dec_last_slice_type(const h264o_dec *d); /* 0 P, 2 I */
/* statistics of the last decoded picture (like h264o_dec_max_level_prefix): the greatest magnitude met in scaling, in the inverse
 * transforms and in the DC transforms (8.5.10 - 8.5.13 demand -2^15 .. 2^15 - 1; -2^15 counts as 2^15 - 1), the greatest |level|,
 * the greatest |mvd_l0| component, the least and greatest vector components used for prediction (quarter samples; 0 when
 * nothing was predicted), and per side the number of predicted partitions (P_Skip macroblocks included) all of whose luma
 * reference samples lie outside the picture */
enum { H264O_DSTAT_MAX_INTERMEDIATE = 0, H264O_DSTAT_MAX_LEVEL, H264O_DSTAT_MAX_MVD, H264O_DSTAT_MV_X_MIN, H264O_DSTAT_MV_X_MAX,
       H264O_DSTAT_MV_Y_MIN, H264O_DSTAT_MV_Y_MAX, H264O_DSTAT_OUT_LEFT, H264O_DSTAT_OUT_RIGHT, H264O_DSTAT_OUT_TOP,
       H264O_DSTAT_OUT_BOTTOM, H264O_DSTAT_COUNT };
int h264o_dec_stat(const h264o_dec *d, int which);
int h264o_dec_last_nal_type(const h264o_dec *d);
/* what the loop filter (8.7) did to the last decoded picture: h264o_dec_dbf() is an array of H264O_DBF_COUNT counters, the filter's
 * own account (the decode does not read it).  kind: 0 luma, 1 chroma; bS 1..4.
 *   tables, H264O_DBF_TABLE(t, kind, bS, index 0..51): by indexA the lines evaluated (bS != 0), filtered (filterSamplesFlag) and
 *     those where a sample changed; by indexB the lines filtered and, luma, those of them with ap < beta / with aq < beta
 *   branch cells, H264O_DBF_CELL(c, kind, bS), lines: rejected by the alpha test alone / the p-side / the q-side beta test alone;
 *     luma bS < 4 the four (ap < beta, aq < beta) combinations (APAQ_00 + 2 * ap + aq); delta clipped at -tc, at +tc, unclipped
 *     and non-zero, zero; the p1 / q1 corrections clipped at -tc0, at +tc0, unclipped; Clip1 active on p0 + delta / q0 - delta at
 *     0 and at 255; luma bS 4 the strong test true with each (ap, aq) combination, and false
 *   contexts, H264O_DBF_CTX + c, lines with bS != 0 of a macroblock edge (IDC2_SLICE_EDGE_ALONE: macroblock edges): qPp != qPq at
 *     a left / top edge and, among those, qPp + qPq odd; an I_PCM macroblock on the p / q side; a chroma line whose Cb and Cr
 *     indexA differ; a side's qPI clipped at 0 / at 51; an edge between slices left alone under idc 2, and one filtered under idc 0
 *     whose slices have different SliceQP_Y; transform_size_8x8_flag differing across the edge; EDGE + 4 * dir + e: lines of
 *     (direction, edge 0..3) */
enum { H264O_DBT_A_EVAL = 0, H264O_DBT_A_FILT, H264O_DBT_A_CHANGED, H264O_DBT_B_FILT, H264O_DBT_B_AP, H264O_DBT_B_AQ, H264O_DBT_COUNT };
enum { H264O_DBC_REJ_ALPHA = 0, H264O_DBC_REJ_P, H264O_DBC_REJ_Q, H264O_DBC_APAQ_00, H264O_DBC_APAQ_01, H264O_DBC_APAQ_10, H264O_DBC_APAQ_11,
       H264O_DBC_DELTA_CLIP_NEG, H264O_DBC_DELTA_CLIP_POS, H264O_DBC_DELTA_UNCLIPPED, H264O_DBC_DELTA_ZERO,
       H264O_DBC_P1_CLIP_NEG, H264O_DBC_P1_CLIP_POS, H264O_DBC_P1_UNCLIPPED, H264O_DBC_Q1_CLIP_NEG, H264O_DBC_Q1_CLIP_POS, H264O_DBC_Q1_UNCLIPPED,
       H264O_DBC_CLIP1_P0_AT_0, H264O_DBC_CLIP1_P0_AT_255, H264O_DBC_CLIP1_Q0_AT_0, H264O_DBC_CLIP1_Q0_AT_255,
       H264O_DBC_STRONG_00, H264O_DBC_STRONG_01, H264O_DBC_STRONG_10, H264O_DBC_STRONG_11, H264O_DBC_STRONG_FALSE, H264O_DBC_COUNT };
enum { H264O_DBX_LEFT_QP_DIFF = 0, H264O_DBX_TOP_QP_DIFF, H264O_DBX_LEFT_QP_ODD, H264O_DBX_TOP_QP_ODD, H264O_DBX_PCM_P, H264O_DBX_PCM_Q,
       H264O_DBX_CBCR_DIFF, H264O_DBX_QPI_CLIP_0, H264O_DBX_QPI_CLIP_51, H264O_DBX_IDC2_SLICE_EDGE_ALONE, H264O_DBX_IDC0_SLICE_EDGE_QP_DIFF,
       H264O_DBX_T8_BESIDE_4X4, H264O_DBX_EDGE, H264O_DBX_COUNT = H264O_DBX_EDGE + 8 };
#define H264O_DBF_TABLE(t, kind, bS, idx) ((((t) * 2 + (kind)) * 4 + (bS) - 1) * 52 + (idx))
#define H264O_DBF_CELLS (H264O_DBT_COUNT * 2 * 4 * 52)
#define H264O_DBF_CELL(c, kind, bS) (H264O_DBF_CELLS + ((c) * 2 + (kind)) * 4 + (bS) - 1)
#define H264O_DBF_CTX (H264O_DBF_CELLS + H264O_DBC_COUNT * 2 * 4)
#define H264O_DBF_COUNT (H264O_DBF_CTX + H264O_DBX_COUNT)
const uint32_t *h264o_dec_dbf(const h264o_dec *d);
int h264o_dec_dbf_count(void);
/* what the prediction (8.3, 8.4.2.2) of the last decoded picture was made of: h264o_dec_pred() is an array of H264O_PRED_COUNT counters,
 * the decoder's own account (the decode does not read it).  Every cell is defined by sample coordinates against the picture and by
 * the availability of 6.4.x.  W, H: the picture's width and height in samples of the plane in question.
 * inter luma, per predicted partition (P_Skip: one of 16x16): xFrac = mvx & 3, yFrac = mvy & 3; on the horizontal axis the window is
 * the columns 8.4.2.2.1 reads, xInt .. xInt + w - 1, with xFrac != 0 xInt - 2 .. xInt + w + 2 (the vertical axis alike), and its
 * relation to 0 .. W - 1 is one of H264O_PRR_*
 *   L_SHAPE [shape H264O_PRS_*][yFrac][xFrac];  L_REF [ref_idx_l0 0..2][yFrac][xFrac];  L_REL [axis 0 x / 1 y][fraction on it][relation]
 *   L_CROSS [axis][fraction][side 0 low / 1 high][columns or rows outside: 1, 2, 3, 4 and more] for the crossing relations (CROSS_BOTH
 *     counts on both sides);  L_CORNER [y side][x side]: both fractions non-zero and the window crosses an edge on either axis
 * inter luma, per 4x4 block of a partition: B_REF [ref_idx_l0][yFrac][xFrac] (its sum: the inter 4x4 blocks of the picture); the
 *   block's own window horizontally inside: B_ALIGN [xInt & 3][xFrac], and with xFrac != 0 B_RDIST [W - 1 - its last column: 0..3, 4 and more]
 * inter luma, per predicted sample: L_CLIP [4 * yFrac + xFrac][intermediate 0 b-type (b, s) / 1 h-type (h, m) / 2 j][Clip1 active at 0 / at 255],
 *   of the intermediates Table 8-12 uses for that position
 * inter chroma, per predicted partition: xFracC = mvx & 7, xIntC = x / 2 + (mvx >> 3), window xIntC .. xIntC + w / 2 - 1 (+ 1 with xFracC != 0)
 *   C_FRAC [yFracC][xFracC];  C_REL [axis][fraction zero / non-zero][relation];  C_CROSS [axis][zero / non-zero][side][samples outside 1, 2, 3, 4 and more]
 *   C_RDIST [samples from the window's last column to the picture's last one, both counted: 1..7, 8 and more], xFracC != 0 and the window horizontally inside
 *   per horizontally adjacent pair of 4x4 luma blocks of one 8x8 quadrant: C_PAIR [0 the same vector / 1 mv >> 3 differs on an axis / 2 only mv & 7 differs],
 *   C_PAIR_MIXED: differing pairs with the 2x2 chroma window of one block inside the picture and the other's not
 * Intra4x4, per block: I4 [Intra4x4PredMode][left | top << 1 | top-left << 2 | top-right << 3 as 8.3.1.2 has them before substitution];
 *   I4_NB [neighbour 0 left, 1 top, 2 top-left, 3 top-right][H264O_PRN_*];  I4_TR_NYD [blkIdx]: top-right not yet decoded;
 *   I4_TR [0 mode 3 / 1 mode 7][0 top-right substituted by p[3, -1] / 1 real]
 * I16, IC [mode][left | top << 1 | top-left << 2] per macroblock (IC: intra_chroma_pred_mode);  IC_DC [chroma4x4BlkIdx][left][top] per plane with
 *   mode 0 (8.3.4);  PLANE_CLIP [0 luma / 1 chroma][Clip1 active at 0 / at 255] per sample of a plane-mode prediction
 * IBI [side 0 left, 1 top, 2 top-left, 3 top-right][coded_block_pattern of the neighbour 0 / non-zero]: intra macroblocks whose prediction
 *   reads samples of an inter macroblock on that side */
enum { H264O_PRS_SKIP = 0, H264O_PRS_16X16, H264O_PRS_16X8, H264O_PRS_8X16, H264O_PRS_8X8, H264O_PRS_8X4, H264O_PRS_4X8, H264O_PRS_4X4 };
enum { H264O_PRR_INSIDE = 0, H264O_PRR_CROSS_LOW, H264O_PRR_CROSS_HIGH, H264O_PRR_BEYOND_LOW, H264O_PRR_BEYOND_HIGH, H264O_PRR_CROSS_BOTH };
enum { H264O_PRN_OUTSIDE = 0, H264O_PRN_OTHER_SLICE, H264O_PRN_NOT_YET_DECODED, H264O_PRN_CONSTRAINED_INTER, H264O_PRN_SAME_MB, H264O_PRN_INTRA_MB,
       H264O_PRN_IPCM_MB, H264O_PRN_INTER_MB };
enum { H264O_PRED_L_SHAPE = 0, H264O_PRED_L_REF = H264O_PRED_L_SHAPE + 8 * 16, H264O_PRED_L_REL = H264O_PRED_L_REF + 3 * 16,
       H264O_PRED_L_CROSS = H264O_PRED_L_REL + 2 * 4 * 6, H264O_PRED_L_CORNER = H264O_PRED_L_CROSS + 2 * 4 * 2 * 4, H264O_PRED_B_REF = H264O_PRED_L_CORNER + 4,
       H264O_PRED_B_ALIGN = H264O_PRED_B_REF + 3 * 16, H264O_PRED_B_RDIST = H264O_PRED_B_ALIGN + 16, H264O_PRED_L_CLIP = H264O_PRED_B_RDIST + 5,
       H264O_PRED_C_FRAC = H264O_PRED_L_CLIP + 16 * 3 * 2, H264O_PRED_C_REL = H264O_PRED_C_FRAC + 64, H264O_PRED_C_CROSS = H264O_PRED_C_REL + 2 * 2 * 6,
       H264O_PRED_C_RDIST = H264O_PRED_C_CROSS + 2 * 2 * 2 * 4, H264O_PRED_C_PAIR = H264O_PRED_C_RDIST + 8, H264O_PRED_C_PAIR_MIXED = H264O_PRED_C_PAIR + 3,
       H264O_PRED_I4 = H264O_PRED_C_PAIR_MIXED + 1, H264O_PRED_I4_NB = H264O_PRED_I4 + 9 * 16, H264O_PRED_I4_TR_NYD = H264O_PRED_I4_NB + 4 * 8,
       H264O_PRED_I4_TR = H264O_PRED_I4_TR_NYD + 16, H264O_PRED_I16 = H264O_PRED_I4_TR + 4, H264O_PRED_IC = H264O_PRED_I16 + 4 * 8,
       H264O_PRED_IC_DC = H264O_PRED_IC + 4 * 8, H264O_PRED_PLANE_CLIP = H264O_PRED_IC_DC + 16, H264O_PRED_IBI = H264O_PRED_PLANE_CLIP + 4,
       H264O_PRED_COUNT = H264O_PRED_IBI + 8 };
const uint32_t *h264o_dec_pred(const h264o_dec *d);
int h264o_dec_pred_count(void);

#ifdef __cplusplus
}
#endif
#endif
