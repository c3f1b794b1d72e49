/*
 * include/mi355x_h264.h -- the drop-in boundary: a plain C ABI over the
 * hand-written HIP (gfx950) H.264 encode path.  No C++ or torch types cross it.
 *
 * Each entry point replaces one use of the OpenH264 vtable that the
 * reference's adapter makes (paths relative to /root/reference):
 *
 *   mi355x_h264_create      <- WelsCreateSVCEncoder + ISVCEncoder::InitializeExt
 *                              + SetOption(ENCODER_OPTION_DATAFORMAT)
 *                              video_codec/VideoEncoderOpenH264.cpp:142, :257, :262
 *                              (decl vendor/openh264/codec_api.h:286, :545)
 *   mi355x_h264_encode      <- ISVCEncoder::EncodeFrame
 *                              video_codec/VideoEncoderOpenH264.cpp:344
 *                              (decl vendor/openh264/codec_api.h:309); the
 *                              SSourcePicture plane/stride triple of :354-365
 *                              becomes the y/u/v + stride arguments, and the
 *                              SFrameBSInfo consumption of :349-350 becomes
 *                              (*out, *out_len)
 *   mi355x_h264_force_idr   <- ISVCEncoder::ForceIntraFrame(true)
 *                              video_codec/VideoEncoderOpenH264.cpp:408
 *                              (decl vendor/openh264/codec_api.h:323)
 *   mi355x_h264_destroy     <- ISVCEncoder::Uninitialize + WelsDestroySVCEncoder
 *                              video_codec/VideoEncoderOpenH264.cpp:382-383
 *
 * The *_device / *_batch entry points are this build's additions for callers
 * whose frames are already resident in HBM (bench.py, multi-stream sharding);
 * the mi355x_h264_debug_* ones expose intermediate device buffers so tests can
 * compare every stage against the CPU oracle.
 *
 * Ownership mirrors the reference: input is caller-owned and
 * only read during the call; the output bitstream lives in encoder-owned
 * (pinned host) memory and stays valid until the next encode / destroy on the
 * same handle.  All functions return 0 on success or a negative MI355X_H264_E_*.
 * Nothing here falls back to a CPU encoder: if no HIP device is usable,
 * mi355x_h264_create fails with MI355X_H264_E_NODEVICE.
 */
#ifndef MI355X_H264_H
#define MI355X_H264_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_H264_ABI_VERSION 3

enum {
    MI355X_H264_OK = 0,
    MI355X_H264_E_ARG = -1,      /* bad argument / unsupported configuration        */
    MI355X_H264_E_NODEVICE = -2, /* no usable HIP device (never a silent CPU path)  */
    MI355X_H264_E_HIP = -3,      /* a HIP runtime call failed (see last_error)      */
    MI355X_H264_E_NOMEM = -4,
    MI355X_H264_E_OVERFLOW = -5, /* a slice coded to more than its payload buffer (twice its luma bytes; only synthetic
                                  * noise at the lowest QPs does): the picture is refused, nothing is written past the
                                  * buffer, and the next picture is coded as an IDR (the refused one is missing from
                                  * the stream and must not be referred to)                                            */
    MI355X_H264_E_INTERNAL = -6
};

enum { MI355X_H264_FRAME_IDR = 1, MI355X_H264_FRAME_P = 3 }; /* EVideoFrameType values, codec_def.h:70,72 */

enum { MI355X_H264_RC_FIXED_QP = 0, MI355X_H264_RC_BITRATE = 1 };
enum { MI355X_H264_INPUT_I420 = 0, MI355X_H264_INPUT_NV12 = 1,
       MI355X_H264_INPUT_RGBA = 2 /* mi355x_h264_stream_open only; mi355x_h264_create refuses it */ };
enum { MI355X_H264_SEARCH_EXHAUSTIVE = 0, MI355X_H264_SEARCH_SEEDED = 1 };

typedef struct mi355x_h264_config {
    uint32_t struct_size;    /* sizeof(mi355x_h264_config), for ABI growth          */
    int32_t width, height;   /* iPicWidth/iPicHeight (ref :235-236); even, 16..4096 */
    int32_t fps;             /* fMaxFrameRate (ref :241): 30 or 60                  */
    int32_t bitrate;         /* iTargetBitrate (ref :239), used when rc_mode == 1   */
    int32_t gop;             /* uiIntraPeriod (ref :242)                            */
    int32_t profile_idc;     /* uiProfileIdc (ref :248-254): 66, 77 or 100          */
    int32_t rc_mode;         /* MI355X_H264_RC_*; the reference preset is BITRATE   */
    int32_t qp;              /* picture QP for FIXED_QP (10..51); initial QP else   */
    int32_t device;          /* HIP device ordinal                                  */
    int32_t disable_deblock; /* iLoopFilterDisableIdc (ref :295), 0 = filter on     */
    int32_t batch;           /* closed GOPs (or independent streams) encoded in lockstep by one instance,
                              * 1..64; > 1 is driven through mi355x_h264_encode_gops_device only      */
    int32_t input_format;    /* layout of pictures handed over in DEVICE memory (encode_device, encode_batch_device,
                              * encode_gops_device): MI355X_H264_INPUT_I420 (default) or MI355X_H264_INPUT_NV12; streams: the
                              * layout of every picture of the stream, MI355X_H264_INPUT_RGBA included (see "streams")   */
    int32_t slices;          /* 0 / 1: one slice per picture (the reference preset, SM_SINGLE_SLICE, ref :247).  n > 1:
                              * n bands of ceil(rows / n) macroblock rows (at least two rows each), one slice NAL
                              * unit per band, disable_deblocking_filter_idc = 2: the bands of a picture
                              * do not depend on one another, their row wavefronts run side by side                  */
    int32_t band_index;      /* slice bands of ONE picture over several GPUs (BASELINE.json configs[4]): */
    int32_t band_count;      /* with band_count > 1 this instance codes only its share of the `slices` slices (a contiguous
                              * run of whole slices, index band_index of band_count); see mi355x_h264_band_*              */
    int32_t refs;            /* iNumRefFrame (ref :290: 1).  0 / 1: one reference frame; 2, 3: the motion search covers the last
                              * `refs` pictures and ref_idx_l0 is coded (BASELINE.json configs[4] asks for 3)                  */
    int32_t search;          /* integer motion search (ABI 3).  MI355X_H264_SEARCH_EXHAUSTIVE: every position of +-16 samples around the
                              * co-located macroblock.  MI355X_H264_SEARCH_SEEDED (what mi355x_h264_default_config sets): the
                              * macroblock's vector in the previous picture, rounded to integer samples, is taken as the integer
                              * winner when it is a strict local minimum of the search cost among its eight integer neighbours -
                              * what a predictor-seeded search does - and the exhaustive pass runs whenever that
                              * test fails.  Costs 0.0 .. 0.2 % bytes at equal PSNR on five of six test contents, 1.3 % at worst
                              * (DESIGN.md section 3); both forms are bit-exact against the oracle's.                          */
} mi355x_h264_config;

typedef struct mi355x_h264_encoder mi355x_h264_encoder;

int mi355x_h264_abi_version(void);
void mi355x_h264_default_config(mi355x_h264_config *cfg);
int mi355x_h264_create(const mi355x_h264_config *cfg, mi355x_h264_encoder **out);
void mi355x_h264_destroy(mi355x_h264_encoder *enc);

/* Encode one I420 picture given as host pointers.  *out receives an Annex-B
 * access unit (SPS+PPS+IDR slice, or one P slice) in encoder-owned memory. */
int mi355x_h264_encode(mi355x_h264_encoder *enc, const uint8_t *y, int y_stride, const uint8_t *u,
                       int u_stride, const uint8_t *v, int v_stride, uint8_t **out, uint32_t *out_len,
                       int *frame_type);

/* Same, with the picture already in device memory as one tightly packed I420
 * buffer (Y, then U, then V; width*height*3/2 bytes). */
int mi355x_h264_encode_device(mi355x_h264_encoder *enc, const void *d_i420, uint8_t **out,
                              uint32_t *out_len, int *frame_type);

/* NV12 ingest (BASELINE.json configs[2]): Y plane followed by one interleaved
 * UV plane.  OpenH264 itself only takes I420 (ref :256,:262); here the kernels read the interleaved
 * chroma rows directly (one 8-byte load + byte permute per four samples): no conversion pass, no extra
 * HBM traffic, and the host never touches the samples.  uv_stride in bytes. */
int mi355x_h264_encode_nv12(mi355x_h264_encoder *enc, const uint8_t *y, int y_stride, const uint8_t *uv,
                            int uv_stride, uint8_t **out, uint32_t *out_len, int *frame_type);
/* tightly packed NV12 in device memory: Y (width*height) then UV (width*height/2) */
int mi355x_h264_encode_nv12_device(mi355x_h264_encoder *enc, const void *d_nv12, uint8_t **out,
                                   uint32_t *out_len, int *frame_type);

/* RGBA ingest (the reference's own interface names the layout only on its decoder side,
 * video_decoder/include/VideoDecoder.h:40-47 PIXEL_FORMAT_RGBA_8888 - no reference ENCODER path takes it, so the conversion
 * is this library's definition, stated in oracle/h264_rgba.c): 8-bit R, G, B, A bytes per sample, alpha ignored.  One
 * conversion kernel writes the I420 picture the encoder then reads: BT.601 studio swing in the usual integer form,
 *   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16,
 *   Cb = ((-38 r - 74 g + 112 b + 128) >> 8) + 128,  Cr = ((112 r - 94 g - 18 b + 128) >> 8) + 128
 * with r, g, b the rounded mean of the four samples of a 2x2 block.  stride in bytes (>= 4 * width).  Batch-1 encoders. */
int mi355x_h264_encode_rgba(mi355x_h264_encoder *enc, const uint8_t *rgba, int stride, uint8_t **out,
                            uint32_t *out_len, int *frame_type);
/* tightly packed RGBA in device memory (4 * width bytes per row) */
int mi355x_h264_encode_rgba_device(mi355x_h264_encoder *enc, const void *d_rgba, uint8_t **out,
                                   uint32_t *out_len, int *frame_type);

/* Encode `count` device-resident pictures back to back; picture i starts at
 * d_frames + i*frame_stride_bytes.  Access units are appended to host_out
 * (capacity out_cap); sizes[i] receives the byte length of picture i.  The
 * host-side finishing of picture i overlaps the GPU work of picture i+1. */
int mi355x_h264_encode_batch_device(mi355x_h264_encoder *enc, const void *d_frames,
                                    size_t frame_stride_bytes, int count, uint8_t *host_out,
                                    size_t out_cap, uint32_t *sizes, size_t *total_len);

/* Lockstep encode of `batch` closed GOPs (config.batch): picture t of GOP g is read from
 * d_frames + g*gop_stride + t*frame_stride (device memory, tight I420).  Every kernel runs once per
 * picture index over all GOPs (grid.y = batch), so the launches are `batch` times larger instead of
 * `batch` times more numerous.  The first picture of every GOP is an IDR; idr_pic_id of GOP g is
 * next + g*step (set_idr_pic_id), so consecutive GOPs concatenate to the serial stream.  GOP g's access
 * units are appended at host_out + g*out_cap_per_gop; sizes[g*frames_per_gop + t], gop_bytes[g]. */
int mi355x_h264_encode_gops_device(mi355x_h264_encoder *enc, const void *d_frames, size_t frame_stride,
                                   size_t gop_stride, int frames_per_gop, uint8_t *host_out,
                                   size_t out_cap_per_gop, uint32_t *sizes, size_t *gop_bytes);

/* ---- slice bands of one picture on several encoder instances / GPUs (config.band_count > 1) ----
 * Every instance is created with the full picture geometry and the same `slices`, and is handed the full source picture
 * (only its band's rows are read).  mi355x_h264_encode* then returns this band's slice NAL units only (SPS/PPS with
 * band 0); the access unit is the concatenation over band_index.  Motion search and compensation of the next picture
 * reach up to 19 sample rows beyond the band, so after every picture the neighbours swap two macroblock rows of
 * reconstruction (the host class does it with one RCCL send/recv pair per neighbour over xGMI):
 *     export(enc, 0, buf) -> send to band_index-1;  export(enc, 1, buf) -> send to band_index+1
 *     import(enc, 0, buf) <- received from band_index-1 (its bottom rows);  import(enc, 1, buf) <- from band_index+1
 * buf: halo_bytes (band_info) of device memory - or of host memory, when the transport between the ranks is a host one.
 * The result equals the stream ONE instance with the same `slices` makes. */
int mi355x_h264_band_info(const mi355x_h264_encoder *enc, int *first_row, int *rows, int *first_slice, int *slices,
                          size_t *halo_bytes);
int mi355x_h264_band_halo_export(mi355x_h264_encoder *enc, int edge, void *d_dst);
int mi355x_h264_band_halo_import(mi355x_h264_encoder *enc, int edge, const void *d_src);

int mi355x_h264_force_idr(mi355x_h264_encoder *enc);
/* picture QP (10..51) for the pictures that follow; the hook the rate controller
 * of the host class drives (RC_BITRATE_MODE, ref :274) */
int mi355x_h264_set_qp(mi355x_h264_encoder *enc, int qp);
/* idr_pic_id of the next IDR picture and its increment per IDR (mod 256).  With closed GOPs
 * sharded over several encoder instances / GPUs (instance i of G: next = i, step = G) the
 * concatenated output equals the serial stream byte for byte. */
int mi355x_h264_set_idr_pic_id(mi355x_h264_encoder *enc, int next, int step);
/* ---- temporal layers: every second P picture non-reference and droppable ----
 * Number the pictures of a GOP from the IDR picture at position 0; config.gop counts all pictures, and a forced IDR picture
 * restarts at position 0.
 *   Layer 0, the even positions: what pictures are without layers, except that "the previous picture" everywhere means the
 *     previous LAYER-0 picture - the reference pictures and their count, frame_num, the ring slot, and the per-macroblock
 *     previous-picture vector of the motion search (seed, rate predictor, "nothing left to code" tests).
 *   Layer 1, the odd positions: a P picture that is no reference picture.  nal_ref_idc is 0, its slice header has no
 *     dec_ref_pic_marking(), its frame_num is PrevRefFrameNum + 1 (7.4.3; the next layer-0 picture carries the same).  It refers to
 *     what a reference picture in its place would refer to, with the same num_ref_idx override and the same search seeds, and is
 *     reconstructed and filtered like any picture - into the ring slot the next layer-0 picture overwrites.  After it, ring
 *     position, frame_num, reference count and motion state are what the layer-0 picture before it left.
 * The picture QP follows one rule for both layers; SPS and PPS do not change by a bit (POC type 2 allows non-reference pictures
 * that do not follow each other), so two-layer and ordinary streams of one geometry share an engine and a lockstep step.  A stream
 * with its nal_ref_idc 0 NAL units removed is the stream an encoder with gop = ceil(gop / 2) writes for the layer-0 pictures alone,
 * byte for byte.  A stream that does not ask for layers is not changed in any way.  frame_type is MI355X_H264_FRAME_P for a
 * layer-1 picture; the layer is read with the two _last_temporal_id calls (0 or 1, of the last finished picture).
 * A refused or failed picture of either layer forces an IDR picture next, as ever.
 * mi355x_h264_set_temporal_layers: 1 or 2, before the encoder's first picture only.  MI355X_H264_E_ARG, before the device is touched:
 * another count, a band instance (band_count > 1: the halo exchange is the caller's) with 2, a call after the first picture; and
 * mi355x_h264_debug_code_syntax on a two-layer encoder.  Streams: MI355X_H264_STREAM_TEMPORAL2 in the flags of the open calls. */
int mi355x_h264_set_temporal_layers(mi355x_h264_encoder *enc, int layers);
int mi355x_h264_last_temporal_id(const mi355x_h264_encoder *enc);
/* ---- intra refresh: a moving all-intra slice band, recovery without an IDR picture ----
 * An encoder or stream with config.slices = n (2 .. 32, and the picture really has n bands: every band two macroblock rows or more)
 * and intra refresh on codes IDR pictures as ever.  Let p = 1, 2, ... count the P pictures since the last IDR picture and
 * k = (p - 1) mod n.  In that P picture
 *   band k is ALL INTRA: every macroblock of it goes to the intra pass without a motion search.  It stays a P slice (mb_type 5..,
 *     every mb_skip_run 0);
 *   bands j < k are CLEAN: the prediction of their macroblocks reads no sample below luma row L = 16 * row_end(k - 1) - 1 of the
 *     reference picture, luma and chroma, under the reads of 8.4.2.2.1 / 8.4.2.2.2.  For a partition at luma row y0 of height hp
 *     with vertical vector vy (quarter samples) the last luma row read is y0 + floor(vy / 4) + hp - 1, plus 3 when vy % 4 != 0, and
 *     is <= L; the last chroma row read is y0 / 2 + floor(vy / 8) + hp / 2 - 1, plus 1 when vy % 8 != 0, and is <= (L + 1) / 2 - 1;
 *   bands j > k are unrestricted.
 * Slices neither predict, filter nor code across their edges, so a decoder that starts at an access unit with k = 0 (or lost
 * pictures before it) has every sample right from the picture with k = n - 1 on, band j from the picture with k = j on.  The access
 * unit with k = 0 starts with a recovery point SEI (NAL type 6, nal_ref_idc 0, payload type 6): recovery_frame_cnt = n - 1,
 * exact_match_flag 1, broken_link_flag 0, changing_slice_group_idc 0.  IDR pictures come as before - by config.gop, on force_idr,
 * on a scene change, after a failed picture - and each restarts p.  A forced macroblock adds 0 to the scene-change statistic.
 * With refresh off nothing differs from an encoder without it.
 * mi355x_h264_set_intra_refresh: on = 0 / 1, before the encoder's first picture only.  MI355X_H264_E_ARG, before the device is
 * touched: slices outside 2 .. 32 or a picture that does not divide into that many bands, refs > 1, two temporal layers (either
 * order of the two calls), a band instance (band_count > 1), a call after the first picture; and mi355x_h264_debug_code_syntax on
 * such an encoder.  Streams: MI355X_H264_STREAM_INTRA_REFRESH in the flags of the open calls, refused on the same grounds.
 * The two _last_refresh_band calls give k of the last finished picture, -1 for an IDR picture or with refresh off.
 * The decoder peer recovers as promised here: mi355x_h264_dec.h, "loss mode".
 * Not built: the encoder repeating SPS / PPS at recovery points (a receiver that joins needs them from elsewhere), refresh with
 * several reference pictures or temporal layers, column refresh, rate control aware of the intra band. */
int mi355x_h264_set_intra_refresh(mi355x_h264_encoder *enc, int on);
int mi355x_h264_last_refresh_band(const mi355x_h264_encoder *enc);
/* Scene-change statistic of the last finished picture, one value per batch item: the sum over the
 * macroblocks that went through motion search of min(final SATD-based motion cost, 16383); 0 for IDR
 * pictures.  The plugin class compares it with a threshold and re-codes the picture as IDR
 * (bEnableSceneChangeDetect = 1 in the reference preset, VideoEncoderOpenH264.cpp:283). */
int mi355x_h264_last_me_cost(const mi355x_h264_encoder *enc, uint32_t *cost);
const char *mi355x_h264_last_error(const mi355x_h264_encoder *enc);

/* coded picture geometry (multiples of 16) */
int mi355x_h264_coded_width(const mi355x_h264_encoder *enc);
int mi355x_h264_coded_height(const mi355x_h264_encoder *enc);

/* ---- test / measurement hooks ---- */
enum {
    MI355X_H264_DBG_RECON_Y = 0,   /* deblocked reconstruction = next reference, coded size */
    MI355X_H264_DBG_RECON_U = 1,
    MI355X_H264_DBG_RECON_V = 2,
    MI355X_H264_DBG_MBINFO = 3,    /* 32 B per macroblock, layout of h264 mbinfo below      */
    MI355X_H264_DBG_LEVELS = 4,    /* 416 int16 per macroblock.  Defined where the picture's syntax reads them (by macroblock type
                                    * and coded_block_pattern, 7.3.5.3); a part whose pattern bit is clear holds whatever an earlier
                                    * picture left there */
    MI355X_H264_DBG_PRE_Y = 5,     /* reconstruction before the loop filter (needs          */
    MI355X_H264_DBG_PRE_U = 6,     /*  mi355x_h264_debug_keep_pre(enc, 1))                  */
    MI355X_H264_DBG_PRE_V = 7,
    MI355X_H264_DBG_MBAUX = 8,     /* 16 B per macroblock: Intra4x4PredMode of the blocks of type-4 macroblocks   */
    MI355X_H264_DBG_MVQ = 9,       /* 8 int16 per macroblock: (x, y) vectors of the four 8x8 quadrants of an inter macroblock */
    MI355X_H264_DBG_SRC = 10       /* the tight source picture of the last picture as it lies in the library's own staging memory, where the
                                    * encoder kernels read it: width * height * 3 / 2 bytes, I420 for I420 and RGBA input (an RGBA
                                    * picture is always converted into staging, from host or device memory: this is what the conversion
                                    * wrote), NV12 for NV12 input.  MI355X_H264_E_ARG, with an error text and the handle as usable as
                                    * before, when there is nothing to read: the last picture was read in place from the caller's device
                                    * memory (I420 / NV12 device pictures, mi355x_h264_encode_batch_device / _gops_device, a picture of
                                    * mi355x_h264_debug_code_syntax), or there has been no picture yet.  Reading it changes nothing
                                    * on the encode path */
};
int mi355x_h264_debug_keep_pre(mi355x_h264_encoder *enc, int on);
/* copies the named device buffer of the last encoded picture (batch item 0) to dst; returns bytes or <0 */
int64_t mi355x_h264_debug_read(mi355x_h264_encoder *enc, int what, void *dst, size_t cap);

/* Codes ONE picture (every batch item's) from GIVEN decisions: the inverse of mi355x_h264_debug_read, the way into the entropy stage
 * for syntax the decision kernels never choose (tests/test_gpu_entropy_random.py).  mbinfo, levels, mvq, mbaux: host arrays in the
 * layouts of MI355X_H264_DBG_MBINFO / _LEVELS / _MVQ / _MBAUX, config.batch items one after the other (an item = all macroblocks of
 * the coded picture); src_i420: config.batch tight I420 pictures of the display size, one after the other - the samples of I_PCM
 * macroblocks are read from there.  The picture goes the way of every other picture - picture type by the same rule (forced IDR,
 * first picture, GOP length), frame_num, idr_pic_id, ring slot and reference count kept the same way - except that the arrays are
 * uploaded where the decision, transform and reconstruction kernels would have run, and that nothing is loop-filtered: boundary
 * strengths, vector prediction and P_Skip, skip runs, both CAVLC passes, the bit scan, packing and the host's finishing run as in
 * mi355x_h264_encode.  An inter macroblock is given as P_L0_16x16 / 16x8 / 8x16 / 8x8 with its vectors in mvq; whether it is written
 * as P_Skip is decided on the device, as always.  What the arrays must respect is what the encoder's own pictures do: one QP (set_qp),
 * ref_idx_l0 of a macroblock in chroma_mode and below the picture's reference count, tc consistent with levels.
 * out / out_len: config.batch entries; item g's access unit, exactly as mi355x_h264_encode returns it, valid until the next call on
 * the handle.  An item that fails (MI355X_H264_E_OVERFLOW: one of its slices outgrew its payload share - there is no I_PCM fallback
 * here) gets out[g] = NULL, out_len[g] = 0, the other items are still delivered, and the first error is returned.
 * The reconstruction ring holds nothing meaningful afterwards: the next mi355x_h264_encode* (or injected) picture is an IDR. */
int mi355x_h264_debug_code_syntax(mi355x_h264_encoder *enc, const void *mbinfo, const void *levels, const void *mvq,
                                  const void *mbaux, const uint8_t *src_i420, uint8_t **out, uint32_t *out_len, int *frame_type);

/* Guard mode of the library's own device and pinned memory (test hook; media_amd/csrc/dev_mem.h).  Every block an encoder, a stream
 * hub, a decoder or a decoder group allocates passes one place.  Off (the default): no launch, no copy and no allocation differs.
 * On: every block of an owner created AFTERWARDS lies between two guard regions of guard_bytes each, filled with a fixed pattern,
 * and - with poison - every block that is not zeroed by design starts filled with 0xCB instead of what the allocator left.  The
 * byte counts the library reports (mi355x_h264_dec_group_last_step) stay the caller's bytes.  A store of a kernel that misses its
 * buffer by less than guard_bytes lands in a guard and is found by the check; a read out of bounds, and a store that misses by
 * more, are not seen.
 *   mi355x_h264_debug_mem_guard: the process-wide switch.  guard_bytes: 0 (off) or a multiple of 4096 up to 1 MiB - anything else
 *     is refused with MI355X_H264_E_ARG and nothing changes.  MI355X_H264_MEM_GUARD=<bytes> and MI355X_H264_MEM_POISON=1 in the
 *     environment give the setting the library starts with.  _get reads the setting (to put it back).
 *   mi355x_h264_debug_mem_check / mi355x_h264_stream_debug_mem_check (and the decoder's, mi355x_h264_dec.h): waits for the owner's
 *     work in flight as its synchronous calls do, compares every guard region with the pattern, and the 256 zeroed bytes behind
 *     every slot of the reconstruction ring with zero.  Returns the number of damaged regions; *regions = regions examined (two per
 *     block, one per ring slot and plane); report: the line "examined blocks=<blocks> slack=<ring slack regions>", then one line per
 *     damaged region, "<block> before|after first=<offset> last=<offset>
 *     bytes=<damaged bytes>", offsets counted from the block's first byte (before: negative).  The stream form covers the hub's
 *     own blocks and the shared engine's, and no other stream of the hub may be in a call meanwhile.  An owner created with the
 *     switch off: MI355X_H264_E_ARG and an error text - "never guarded" is not "intact".
 *   mi355x_h264_debug_mem_tally: every block is checked once more when it is freed (destroy, a staging buffer that grows, a
 *     decoder's change of size); the damaged regions found there are counted process-wide: returns the count, reset != 0 clears
 *     it.  With MI355X_H264_MEM_GUARD_LOG=<file> every damaged region found while freeing is also appended to the file as one
 *     line of the report's form: a run of a whole suite under the environment variables is clean when the file stays absent.
 *   mi355x_h264_debug_mem_poke: sets ONE byte of a guard region from the host (hipMemset, or a store for pinned memory: no kernel
 *     runs), so that a test can see the check report it.  block: the name of a block (the member it was allocated for, as the
 *     source spells it: "d_slotcode", "S.d_bitbuf", "d_plane_base[0]"; the first of that name) or "#N", block N in allocation
 *     order ("#0" the first, "#-1" the last).  offset: from the block's first byte, inside a guard region - any other is refused
 *     with MI355X_H264_E_ARG.  value 0..255, or -1: the pattern's byte is put back. */
int mi355x_h264_debug_mem_guard(int64_t guard_bytes, int poison);
int mi355x_h264_debug_mem_guard_get(int64_t *guard_bytes, int *poison);
int64_t mi355x_h264_debug_mem_tally(int reset);
int mi355x_h264_debug_mem_check(mi355x_h264_encoder *enc, int *regions, char *report, size_t cap);
int mi355x_h264_debug_mem_poke(mi355x_h264_encoder *enc, const char *block, int64_t offset, int value);

/* ---- streams (ABI 3): many encoders of one geometry, one picture per call each, sharing one engine ----
 * The reference's operating mode is one VideoEncoder object per cloud-phone stream, each driven by its own thread with one
 * EncodeOneFrame per tick (/root/reference/video_codec/VideoEncoderOpenH264.cpp:304-352).  A stream is such an encoder whose
 * pictures are coded together with the pictures other streams of the same geometry (size, fps, profile, slices, filter switch,
 * device) deliver at about the same time: ONE lockstep launch sequence per step instead of one per stream, every picture with
 * its own QP, picture type, frame_num and reference pictures.  mi355x_h264_stream_encode is synchronous and may be called from
 * one thread per stream concurrently; the output is bit-for-bit what mi355x_h264_create / mi355x_h264_encode with the same
 * config and the same QP sequence produce (tests/test_gpu_streams.py).
 * Reference pictures: mi355x_h264_stream_open takes refs <= 1 and refuses more (its contract since ABI 3);
 * mi355x_h264_stream_open_ex with MI355X_H264_STREAM_MULTIREF honours refs 2 / 3 (tests/test_gpu_stream_refs.py).  Streams share an
 * engine only with streams of the same refs (0 and 1 are the same), and every position of a shared step has its own number of
 * usable reference pictures, min(refs, pictures since ITS stream's IDR).  An engine holds refs + 1 reconstructions per stream slot:
 * (refs + 1) * MI355X_H264_HUB_ITEMS * 1.5 * coded width * coded height bytes - at 1920x1088 and 32 slots 200 MB with one
 * reference picture, 300 MB with two, 400 MB with three - allocated when the engine's first stream opens.
 * *out stays valid until the stream's next encode / close.  MI355X_H264_HUB_ITEMS (default 32) streams share an engine;
 * MI355X_H264_HUB_WINDOW_US (default 200): how long a step waits for pictures that are already being uploaded. */
typedef struct mi355x_h264_stream mi355x_h264_stream;
int mi355x_h264_stream_open(const mi355x_h264_config *cfg, mi355x_h264_stream **out);
/* mi355x_h264_stream_open with flags.  flags 0: exactly mi355x_h264_stream_open.  MI355X_H264_STREAM_MULTIREF: cfg->refs 2 / 3 is
 * honoured (with refs <= 1 the stream is an ordinary one and shares the engine of mi355x_h264_stream_open streams of its geometry).
 * Unknown flag bits, refs > 3, band_count > 1 and batch > 1 return MI355X_H264_E_ARG before the device is touched.  Every other
 * stream call works unchanged on the stream. */
enum { MI355X_H264_STREAM_MULTIREF = 1,     /* cfg->refs 2 / 3 is honoured */
       MI355X_H264_STREAM_TEMPORAL2 = 8,    /* two temporal layers (above, "temporal layers"); in _open_ex, _open_scaled and _open_colour.
                                             * (Bits 1 and 2 stay unknown bits: callers and tests rely on their being refused.) */
       MI355X_H264_STREAM_INTRA_REFRESH = 32 };   /* intra refresh over the cfg->slices bands (above, "intra refresh"); in the same three
                                                   * calls.  (Bit 4 stays an unknown bit too.) */
int mi355x_h264_stream_last_refresh_band(const mi355x_h264_stream *s);   /* all-intra band of the stream's last finished picture, -1: none */
int mi355x_h264_stream_open_ex(const mi355x_h264_config *cfg, uint32_t flags, mi355x_h264_stream **out);
int mi355x_h264_stream_last_temporal_id(const mi355x_h264_stream *s);   /* temporal layer of the stream's last finished picture */
void mi355x_h264_stream_close(mi355x_h264_stream *s);
int mi355x_h264_stream_encode(mi355x_h264_stream *s, const uint8_t *y, int y_stride, const uint8_t *u, int u_stride,
                              const uint8_t *v, int v_stride, uint8_t **out, uint32_t *out_len, int *frame_type);
/* Layouts and device-resident pictures (tests/test_gpu_stream_inputs.py).  config.input_format names the layout of EVERY picture of
 * the stream - MI355X_H264_INPUT_I420, _NV12 or _RGBA - and streams share an engine only with streams of the same layout.
 * mi355x_h264_stream_encode takes host I420 planes, _encode_nv12 host NV12 (arguments as mi355x_h264_encode_nv12), _encode_rgba
 * host RGBA (as mi355x_h264_encode_rgba; the conversion is the one stated there, one launch for all RGBA pictures of a step).
 * mi355x_h264_stream_encode_device takes ONE tight picture in the stream's layout (I420: Y, U, V; NV12: Y, UV; RGBA: 4 * width
 * bytes per row) in device memory of the stream's device.  Host and device calls may alternate freely on one stream; the output is
 * the same bytes either way.  A call whose form is not the stream's layout (host I420 planes to an NV12 stream, ...) returns
 * MI355X_H264_E_ARG, sets the stream's error text and leaves the stream as it was.
 * Contract of the device form:
 *   - the picture is only read, and only during the call.  I420 and NV12 pictures are read where they lie by the encoder kernels
 *     themselves (no copy is made); an RGBA picture is read once, by the conversion kernel;
 *   - the call does not synchronise with the caller's own HIP streams: whatever writes the picture must have completed;
 *   - alignment: an RGBA picture must start on a multiple of 8 bytes (the conversion loads 8 bytes per lane; less is refused with
 *     MI355X_H264_E_ARG).  I420 and NV12 pictures may start on any byte - every source load of the kernels tests its own address
 *     and takes single bytes when it is not a multiple of 4 (NV12 chroma: 8) - but only pictures that start on a multiple of 8
 *     bytes and whose width is a multiple of 4 are read at full speed.  These are the requirements of mi355x_h264_encode_device
 *     and mi355x_h264_encode_rgba_device as well. */
int mi355x_h264_stream_encode_device(mi355x_h264_stream *s, const void *d_pic, uint8_t **out, uint32_t *out_len, int *frame_type);
int mi355x_h264_stream_encode_nv12(mi355x_h264_stream *s, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                                   uint8_t **out, uint32_t *out_len, int *frame_type);
int mi355x_h264_stream_encode_rgba(mi355x_h264_stream *s, const uint8_t *rgba, int stride, uint8_t **out, uint32_t *out_len,
                                   int *frame_type);
/* Damage tiles (tests/test_gpu_damage.py; media_amd/csrc/damage.h, k_patch.h; restated in tests/damage.py): a host call that
 * transfers only the tiles of the picture that differ from the stream's previous picture.  The access units, the reconstruction
 * and the quality records are byte for byte those of the ordinary call with the picture that is encoded (below).
 *   Grid: tiles of 64 x 16 luma samples at multiples of (64, 16) over the SOURCE picture (mi355x_h264_stream_source_width x
 *     _height); tile index = row of tiles * tiles per row + column.  Tiles at the right and bottom edge are partial.  A tile's
 *     bytes: I420 64 x 16 Y, then 32 x 8 U, then 32 x 8 V (1536); NV12 64 x 16 Y, then 64 x 8 of the interleaved plane (1536);
 *     RGBA 64 x 16 x 4 (4096).
 *   Damage set, caller rectangles {x, y, w, h} in luma samples: every tile a rectangle touches after clipping to the picture; an
 *     empty rectangle or one wholly outside adds nothing; n == 0: nothing changed.  n < 0 (other than the sentinel), n > 0 with
 *     null rects, rects with the sentinel, or a negative w / h: MI355X_H264_E_ARG, and the stream stays as it was.
 *   Damage set, n == MI355X_H264_DAMAGE_DETECT with null rects: every tile with at least one byte inside the picture that differs
 *     from the previous picture (the library compares while it copies; the caller's stride padding is never read).
 *   The picture that is encoded: the stream's previous picture with the damaged tiles replaced from the caller's picture.  With
 *     detect that is exactly the caller's picture; with rectangles that miss a change it is the stated composition, not the
 *     caller's picture.
 *   Slot validity: every stream has a flag "the staging slot holds the previous picture".  A host call (ordinary or damage) that
 *     succeeded sets it; it is clear at open, after every mi355x_h264_stream_encode_device call and after any call that failed
 *     behind the argument checks (its upload or its step may have left the slot half written).  A call refused with
 *     MI355X_H264_E_ARG changes nothing.  With the flag clear a damage call is an ordinary whole upload of the caller's picture,
 *     whatever its rectangles say - the first picture of a stream always goes whole.
 *   Payload: 16-byte header {uint32 magic "DAMG", layout, tiles, bytes per tile}, the tiles' uint32 indices in ascending order,
 *     zeros up to a multiple of 16, the tiles at their full nominal size (bytes of a partial tile outside the picture are
 *     unspecified and never stored): payload = ((16 + 4 * tiles + 15) & ~15) + tiles * bytes per tile.  It goes over the link in
 *     ONE transfer, and one kernel launch per step (k_patch_step) writes the tiles of all its pictures into their slots.
 *   Fallback: the call goes patched when 0 < payload < the tight picture's bytes (w * h * 3 / 2, RGBA w * h * 4); with payload >=
 *     picture the picture that is encoded goes whole in one transfer; with no damaged tile nothing is transferred or patched and
 *     the picture is encoded from the slot as it is.
 * The ordinary calls are untouched: they transfer whole pictures.  Not on the direct mi355x_h264_encode* path or the batch calls. */
typedef struct mi355x_h264_rect { int32_t x, y, w, h; } mi355x_h264_rect;
#define MI355X_H264_DAMAGE_DETECT (-0x44414D47)   /* as n, with null rects: the library finds the damage */
enum { MI355X_H264_UPLOAD_WHOLE = 0,      /* the whole picture went over the link                                      */
       MI355X_H264_UPLOAD_PATCHED = 1,    /* a payload of damaged tiles                                                */
       MI355X_H264_UPLOAD_NOTHING = 2,    /* no tile was damaged: nothing went                                         */
       MI355X_H264_UPLOAD_IN_PLACE = 3 }; /* mi355x_h264_stream_encode_device: the picture was read where it lay       */
int mi355x_h264_stream_encode_damage(mi355x_h264_stream *s, const uint8_t *y, int y_stride, const uint8_t *u, int u_stride,
                                     const uint8_t *v, int v_stride, const mi355x_h264_rect *rects, int n,
                                     uint8_t **out, uint32_t *out_len, int *frame_type);
int mi355x_h264_stream_encode_nv12_damage(mi355x_h264_stream *s, const uint8_t *y, int y_stride, const uint8_t *uv, int uv_stride,
                                          const mi355x_h264_rect *rects, int n, uint8_t **out, uint32_t *out_len, int *frame_type);
int mi355x_h264_stream_encode_rgba_damage(mi355x_h264_stream *s, const uint8_t *rgba, int stride, const mi355x_h264_rect *rects, int n,
                                          uint8_t **out, uint32_t *out_len, int *frame_type);
/* The stream's last picture that got past the argument checks: bytes put on the link for it; damaged tiles (a whole upload
 * that had no damage set - an ordinary call, or a damage call on an invalid slot - counts every tile; in place: 0); tiles of the
 * grid; MI355X_H264_UPLOAD_*.  Any pointer may be null.  Before the first picture: 0, 0, the grid, WHOLE. */
int mi355x_h264_stream_last_upload(const mi355x_h264_stream *s, uint64_t *bytes, uint32_t *tiles, uint32_t *tiles_total, int *mode);
/* test hook: k_patch_step launches of the stream's engine so far, and the tiles they wrote */
int mi355x_h264_stream_debug_patch_stats(const mi355x_h264_stream *s, uint64_t *launches, uint64_t *tiles);
int mi355x_h264_stream_set_qp(mi355x_h264_stream *s, int qp);            /* as mi355x_h264_set_qp            */
int mi355x_h264_stream_force_idr(mi355x_h264_stream *s);                 /* as mi355x_h264_force_idr         */
int mi355x_h264_stream_set_idr_pic_id(mi355x_h264_stream *s, int next);  /* idr_pic_id of the next IDR       */
int mi355x_h264_stream_last_me_cost(const mi355x_h264_stream *s, uint32_t *cost);   /* as mi355x_h264_last_me_cost */
const char *mi355x_h264_stream_last_error(const mi355x_h264_stream *s);
int mi355x_h264_stream_coded_width(const mi355x_h264_stream *s);
int mi355x_h264_stream_coded_height(const mi355x_h264_stream *s);
/* Scaled streams (tests/test_gpu_scale.py): pictures of src_width x src_height are resampled on the device to the coded size,
 * cfg->width x cfg->height, by one launch per lockstep step in front of the first kernel that reads samples
 * (k_scale_to_i420_step); from there on the picture takes the path of every other stream.  `flags` are those of
 * mi355x_h264_stream_open_ex (MI355X_H264_STREAM_MULTIREF combines with scaling).  src == (cfg->width, cfg->height) gives exactly
 * the stream mi355x_h264_stream_open_ex gives, sharing its engine; streams share an engine only with streams of the same source
 * size.  Refused with MI355X_H264_E_ARG before the device is touched: an odd source size, one outside 16 .. 4096, one smaller than
 * the coded size or more than 4 times it in either dimension, and everything mi355x_h264_stream_open_ex refuses.
 * Every mi355x_h264_stream_encode* call of such a stream takes pictures of the SOURCE size (strides are checked against the source
 * width; the device form takes one tight source picture, read where it lies during the call, nothing copied and nothing waited
 * for; it may start on any byte - RGBA: on 8 - and is read at full speed from multiples of 16).  MI355X_H264_DBG_SRC returns the
 * resampled staging picture, width * height * 3 / 2 bytes of I420 for every layout, and the quality report's `src` is that picture.
 * The arithmetic (this library's own definition; tests/scale.py restates it in numpy).  Area (box) resampling of a plane of
 * SW x SH samples to W x H, W <= SW <= 4 W and H <= SH <= 4 H:
 *   - per dimension, result sample x covers [x * SW, (x + 1) * SW) on an axis where source sample i covers [i * W, (i + 1) * W);
 *     the weight wx(x, i) is the integer length of the overlap.  The weights of one result sample sum to SW, and at most 5 source
 *     samples are touched;
 *   - out(x, y) = floor((N + (D >> 1)) / D) with N = sum_j sum_i wx(x, i) * wy(y, j) * src(j, i) and D = SW * SH: the exact
 *     weighted mean rounded to nearest, halves up (an odd D has no ties).  Nothing is rounded between the horizontal and the
 *     vertical sum.  N + (D >> 1) < 2^32 up to 4096 x 4096, and the division is exact (a multiplier the host computes per plane);
 *   - I420: Y is resampled SW x SH -> W x H, U and V each SW/2 x SH/2 -> W/2 x H/2.  NV12: the same, the chroma samples taken from
 *     the interleaved plane.  RGBA: R, G and B are each resampled as a plane (alpha is ignored), and the resampled picture goes
 *     through the RGBA arithmetic stated at mi355x_h264_encode_rgba, unchanged.  2 : 1 in both dimensions is (a + b + c + d + 2) >> 2. */
int mi355x_h264_stream_open_scaled(const mi355x_h264_config *cfg, uint32_t flags, int src_width, int src_height,
                                   mi355x_h264_stream **out);
int mi355x_h264_stream_source_width(const mi355x_h264_stream *s);    /* the size of the pictures the calls take: the coded   */
int mi355x_h264_stream_source_height(const mi355x_h264_stream *s);   /* size for streams that do not scale                   */
/* Test hooks.  mi355x_h264_stream_debug_read: what mi355x_h264_debug_read gives for an encoder (every MI355X_H264_DBG_* value), of the
 * stream's own batch item after the stream's last picture; returns bytes or < 0.  The stream's calls are synchronous and nothing
 * rewrites a stream's arrays before its next call, so other streams may go on encoding meanwhile.
 * MI355X_H264_DBG_PRE_Y / _U / _V need mi355x_h264_stream_debug_keep_pre(s, 1) before the picture: the switch belongs to the shared
 * engine, so it holds for EVERY stream of s's geometry that shares it (and ends with the engine, when its last stream closes).
 * On: every step copies its pictures' planes aside in front of the loop filter (device-to-device copies on the step's HIP
 * stream, into memory every engine owns anyway).  Off (the default): no launch, no copy and no allocation differs. */
int64_t mi355x_h264_stream_debug_read(mi355x_h264_stream *s, int what, void *dst, size_t cap);
int mi355x_h264_stream_debug_keep_pre(mi355x_h264_stream *s, int on);
/* mi355x_h264_debug_mem_check (above) for the blocks of the stream's hub and of the engine its streams share */
int mi355x_h264_stream_debug_mem_check(mi355x_h264_stream *s, int *regions, char *report, size_t cap);
/* Which lockstep step coded the stream's last picture: the step's serial number on the stream's engine (1, 2, ..; steps of
 * one engine are numbered in the order they were gathered), the number of pictures the step carried, this picture's position
 * among them (0 .. pictures - 1: the grid index the indirect kernels saw, not the batch item) and whether it was an IDR
 * step.  Two streams of one geometry (and at most 32 open) that report the same serial were coded by the same launches.
 * Any out-pointer may be null.  serial 0: no picture yet. */
int mi355x_h264_stream_debug_last_step(const mi355x_h264_stream *s, uint64_t *serial, int *pictures, int *position, int *idr);
/* how the stream's engine has been batching: steps launched, pictures coded, largest step, streams open on it */
int mi355x_h264_stream_hub_stats(const mi355x_h264_stream *s, uint64_t *steps, uint64_t *pictures, uint64_t *max_batch,
                                 int *open_streams);

/* ---- colour description (tests/colour.py restates it; tests/test_colour_oracle.py checks the claims over the whole cube) ----
 * Which matrix and which range the samples of a stream have, chosen by the caller and written into the sequence parameter set's
 * VUI.  A stream opened without a description (every call above) is BT.601 studio swing as stated at mi355x_h264_encode_rgba and
 * says nothing: its SPS has vui_parameters_present_flag = 0 and stays bit for bit what it was.
 * RGBA ingest, four variants of one form (r, g, b: the rounded 2x2 means; every result clipped to 0..255):
 *   Y = ((a R + b G + c B + 128) >> 8) + o,  Cb, Cr = ((d r + e g + f b + 128) >> 8) + 128
 *     variant          Y (a, b, c, o)      Cb (d, e, f)      Cr (d, e, f)
 *     BT.601 limited   66, 129, 25, 16     -38, -74, 112     112,  -94, -18     (the undescribed arithmetic, unchanged)
 *     BT.709 limited   47, 157, 16, 16     -26, -86, 112     112, -102, -10
 *     BT.601 full      77, 150, 29,  0     -43, -85, 128     128, -107, -21
 *     BT.709 full      54, 183, 19,  0     -29, -99, 128     128, -116, -12
 * Every chroma row sums to 0 (grey gives 128, 128); the limited forms stay inside 16..235 / 16..240 without the clip; the full
 * forms reach 256 in chroma (and nothing else leaves 0..255), so the clip is needed there.
 * The way out (the decoder's RGBA layout, include/mi355x_h264_dec.h) has the matching four:
 *   c = m (Y - o), d = U - 128, e = V - 128,
 *   R = clip255((c + rv e + 128) >> 8), G = clip255((c + gu d + gv e + 128) >> 8), B = clip255((c + bu d + 128) >> 8)
 *     variant          m, o      rv    gu, gv        bu
 *     BT.601 limited   298, 16   409   -100, -208    516
 *     BT.709 limited   298, 16   459    -55, -136    541
 *     BT.601 full      256,  0   359    -88, -183    454
 *     BT.709 full      256,  0   403    -48, -120    475
 * The VUI of a described stream, in order: no aspect ratio, no overscan; video_signal_type (video_format 5, video_full_range_flag,
 * colour_primaries / transfer_characteristics 1 / 1 for BT.709 and 6 / 6 for BT.601, matrix_coefficients = matrix);
 * chroma_loc_info (both types 1: the 2x2 mean makes centre-sited chroma) for streams of RGBA input only; timing_info
 * (num_units_in_tick 1, time_scale 2 * fps, fixed_frame_rate_flag 1); no HRD, no pic_struct; bitstream_restriction (vectors over
 * picture boundaries 1, both denominators 0, both log2_max_mv_length 16, max_num_reorder_frames 0, max_dec_frame_buffering = the
 * number of reference pictures).
 * For RGBA input the description selects the conversion; for I420 and NV12 input it only says what the caller's samples are, and
 * no sample is touched. */
enum { MI355X_H264_MATRIX_BT709 = 1, MI355X_H264_MATRIX_BT601 = 6 };   /* matrix_coefficients, Table E-5 */
typedef struct mi355x_h264_colour {
    uint32_t struct_size;   /* sizeof(mi355x_h264_colour) */
    int32_t matrix;         /* MI355X_H264_MATRIX_BT709 or MI355X_H264_MATRIX_BT601 */
    int32_t full_range;     /* 0: studio swing, 1: full range */
} mi355x_h264_colour;
/* mi355x_h264_stream_open_scaled plus the description.  A null description gives exactly the mi355x_h264_stream_open_scaled
 * stream, on its engine.  Streams share an engine only with streams of the same description, and a described stream never shares
 * one with an undescribed stream, even where both are BT.601 limited: their parameter sets differ.  Refused with MI355X_H264_E_ARG
 * before the device is touched: a matrix other than the two above, full_range outside 0 / 1, a wrong struct_size, and everything
 * mi355x_h264_stream_open_scaled refuses.  The description of an open stream cannot be changed. */
int mi355x_h264_stream_open_colour(const mi355x_h264_config *cfg, uint32_t flags, int src_width, int src_height,
                                   const mi355x_h264_colour *colour, mi355x_h264_stream **out);
/* mi355x_h264_create plus the description (a null one: exactly mi355x_h264_create).  mi355x_h264_encode_rgba(_device) converts with
 * the described variant.  The layout of an encoder's pictures is the call's, not the handle's, so its VUI carries no chroma_loc_info. */
int mi355x_h264_create_colour(const mi355x_h264_config *cfg, const mi355x_h264_colour *colour, mi355x_h264_encoder **out);
/* the description the handle was opened with: returns 1 and fills *out, or 0 (undescribed; *out is BT.601 limited, what the
 * conversion then is), or MI355X_H264_E_ARG for a null argument */
int mi355x_h264_stream_colour(const mi355x_h264_stream *s, mi355x_h264_colour *out);
int mi355x_h264_colour_of(const mi355x_h264_encoder *enc, mi355x_h264_colour *out);

/* per-kernel device time accumulated since the last reset, measured with HIP
 * events on the encoder's own stream */
enum {
    MI355X_H264_K_ME = 0,       /* motion search (SAD integer + SATD sub-pel)      */
    MI355X_H264_K_PMB = 1,      /* residual + fDCT + quant + dequant + iDCT + recon (k_tq / k_tq8; the MC moved into the search) */
    MI355X_H264_K_INTRA = 2,    /* Intra16x16 wavefront                            */
    MI355X_H264_K_CAVLC = 3,    /* entropy coding + packing                        */
    MI355X_H264_K_DEBLOCK = 4,  /* loop filter wavefront                           */
    MI355X_H264_K_COUNT = 5
};
typedef struct mi355x_h264_stats {
    double ms[MI355X_H264_K_COUNT];       /* summed device milliseconds           */
    uint64_t launches[MI355X_H264_K_COUNT];
    uint64_t mbs[MI355X_H264_K_COUNT];    /* macroblocks processed by that kernel */
    uint64_t frames;
    /* what the P pictures' macroblocks became (counted on the device by the entropy stage, always on; ABI 3):
     * p_mbs      macroblocks of P pictures;
     * me_searched_mbs  of those, the ones k_me's "nothing left to code" tests did NOT settle - the search, the
     *            sub-sample refinement and the prediction write ran for them;
     * tq_coded_mbs     of those, the ones k_tq / k_tq8 coded (searched, and not handed to the intra pass): the
     *            macroblocks the transform kernel loads and stores samples and levels for.  bench.py prices the
     *            roofline of the two kernels on these counts, not on the launch geometry. */
    uint64_t p_mbs, me_searched_mbs, tq_coded_mbs;
} mi355x_h264_stats;
int mi355x_h264_stats_enable(mi355x_h264_encoder *enc, int on);
int mi355x_h264_stats_read(mi355x_h264_encoder *enc, mi355x_h264_stats *out, int reset);

/* ---- quality report: the sum of squared errors (SSE) of every coded picture, per plane and per macroblock ----
 * Definition.  Each of the three planes is compared sample by sample, Y, Cb and Cr reported in the order Y, U, V: the
 * difference (src - rec) is squared and summed.
 *   src  the picture the encoder kernels read: for I420 and NV12 input the caller's samples, for RGBA input the I420 staging
 *        picture the conversion kernel (k_rgba_to_i420 / k_rgba_to_i420_step) wrote; for a scaled stream
 *        (mi355x_h264_stream_open_scaled) the resampled I420 staging picture of the coded size, whatever the layout;
 *   rec  the reconstruction that becomes the next reference, after the loop filter; a picture that is not filtered
 *        (disable_deblock, or a picture with an I_PCM macroblock) is compared as it stands.
 * Only display samples count: luma x < width, y < height; chroma x < width / 2, y < height / 2.  The replicated columns and rows of
 * the coded size never count.  A band instance (band_count > 1) counts the macroblock rows of its own band only, so the sum over
 * the instances equals what one instance reports.
 * Per picture: sse[3], 64 bits per plane (32 are not enough: one 1080p picture of noise at QP 51 has a luma SSE above 2^32), and a
 * map[rows][columns of macroblocks] of uint32_t, each entry the macroblock's SSE over its display samples, all three planes added
 * (at most 384 * 65025); entries outside a band instance's band are 0, and the sum of the map is sse[0] + sse[1] + sse[2].
 * All arithmetic on the device is integer: no float is computed, summed or returned, so the result is exact whatever the order of
 * summation.  PSNR = 10 * log10(255^2 * samples / sse) is the caller's to compute (an SSE of 0: infinite).
 * The switch only observes: access units, mi355x_h264_debug_read results and statistics are the same bytes with it on or off.  Off
 * (the default): no launch, no copy and no allocation differs; the result arrays come with the first enable.  On: one kernel
 * (k_sse) per step, beside the entropy coder and off the chain to the next picture's motion search; its results are complete when
 * the call returns.  MI355X_H264_QUALITY=1 in the environment turns the switch on when an engine is created. */
typedef struct mi355x_h264_quality {
    uint64_t sse[3], samples[3];   /* Y, U, V; samples: what was compared (a band: its rows) */
    uint32_t bytes, qp, frame_type, valid;   /* of the access unit; valid 0: nothing was compared */
} mi355x_h264_quality;
int mi355x_h264_quality_enable(mi355x_h264_encoder *enc, int on);   /* from the next picture on */
/* records of every picture of the last call, in the order of sizes[]: config.batch entries after a one-picture call,
 * count after encode_batch_device, batch * frames_per_gop after encode_gops_device; returns entries or < 0.  cap: entries dst has
 * room for.  valid = 0 marks a picture refused with MI355X_H264_E_OVERFLOW and a picture of mi355x_h264_debug_code_syntax (whose
 * ring holds nothing meaningful); the record is present.  Nothing to read (the switch was off for the last call, no picture yet):
 * MI355X_H264_E_ARG with an error text, the handle as usable as before. */
int64_t mi355x_h264_quality_read(mi355x_h264_encoder *enc, mi355x_h264_quality *dst, size_t cap);
/* the map of the last picture of batch item `item`: coded height / 16 rows of coded width / 16 entries; cap: entries dst has room
 * for; returns entries or < 0 */
int64_t mi355x_h264_quality_map(mi355x_h264_encoder *enc, int item, uint32_t *dst, size_t cap);
/* Streams: the switch belongs to the shared engine, as mi355x_h264_stream_debug_keep_pre's does - it holds for every stream that
 * shares it and ends with the engine.  last_quality / quality_map: of the stream's own last picture. */
int mi355x_h264_stream_quality_enable(mi355x_h264_stream *s, int on);
int mi355x_h264_stream_last_quality(const mi355x_h264_stream *s, mi355x_h264_quality *out);
int64_t mi355x_h264_stream_quality_map(mi355x_h264_stream *s, uint32_t *dst, size_t cap);

/* ---- quality report: SSIM per plane and per macroblock, beside the SSE (tests/ssim.py restates this text in numpy) ----
 * Definition.  src, rec, "display samples" and the plane order Y, U, V are those of the SSE definition above.  A plane is W x H
 * display samples; the chroma planes are width / 2 x height / 2, which may be odd.
 * Windows.  A window is 8x8 samples with its origin at (4i, 4j).  It counts when it lies wholly inside the plane's display samples:
 * 4i + 8 <= W and 4j + 8 <= H, so a plane has (W / 4 - 1) * (H / 4 - 1) windows (integer division): a 16x16 picture has 9 luma
 * windows and one per chroma plane.  A window is never shortened.  A band instance (band_count > 1) counts the windows whose
 * origin row lies in its own macroblock rows and whose last row does too: its limit is min(H, 16 * (row0 + rows)) for luma and
 * min(H / 2, 8 * (row0 + rows)) for chroma.  Windows that straddle two bands belong to nobody: UNLIKE the SSE, the band records do
 * NOT add up to the single instance's; windows[] says how many were counted.
 * Per window, all integers, the sums over its 64 samples:
 *   s1 = sum src, s2 = sum rec, ss = sum (src^2 + rec^2), s12 = sum src * rec
 *   vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2
 *   C1 = 416, C2 = 235963   (the usual (0.01 * 255)^2 * 64 and (0.03 * 255)^2 * 64 * 63, rounded)
 *   l = floor(((2 s1 s2 + C1) << 16) / (s1^2 + s2^2 + C1))      in 0 .. 65536
 *   c = floor(((2 covar + C2) << 16) / (vars + C2))             in -65535 .. 65536; floor, not truncation: the numerator can be negative
 *   q = (l * c) >> 16                                           a 64-bit product, an arithmetic shift
 * Every term before the shifts fits 31 bits, the shifted numerators stay below 2^47, 2 |covar| <= vars.  q / 65536 is within 4.6e-5
 * of the floating-point SSIM of the window.  Identical windows: 65536, 65536, 65536; constant 100 against constant 110: 65239,
 * 65536, 65239; constant 0 against 255: 0, 65536, 0; 32 samples of 0 and 32 of 255 against its inverse: 65536, -65305, -65305.
 * Per picture: sum[3], int64, the sum of q over the plane's windows; windows[3], the window count per plane; a luma map
 * int32_t [rows][columns of macroblocks], each entry the sum of q of the luma windows whose ORIGIN lies in the macroblock (at
 * most 16 windows, so an entry stays inside +-2^20), 0 outside a band instance's band; the map adds up to sum[0].  The mean SSIM of a
 * plane is sum / (65536 * windows): the caller's to compute, as PSNR is.  The device computes, sums and returns no float.
 * The SSIM record accompanies the SSE record, which carries bytes, QP and type: metrics = MI355X_H264_QUALITY_SSE (exactly what
 * mi355x_h264_quality_enable(enc, 1) does), SSE | SSIM (both), or 0 (off); SSIM alone and any other bit: MI355X_H264_E_ARG.
 * mi355x_h264_quality_enable(enc, on) equals _ex(enc, on ? 1 : 0).  With SSIM not asked for nothing differs: no launch, copy,
 * allocation, byte or record; k_ssim's pinned arrays come with the first enable that asks for it.  On: one more kernel (k_ssim)
 * behind k_sse, off the chain like it.  MI355X_H264_QUALITY=3 in the environment turns both on when an engine is created.
 * Records are read like the SSE records and in their order; an injected or refused picture has valid = 0; nothing to read (SSIM was
 * not on for the last call, no picture yet), null handles and a small cap behave as their SSE counterparts do. */
enum { MI355X_H264_QUALITY_SSE = 1, MI355X_H264_QUALITY_SSIM = 2 };
typedef struct mi355x_h264_ssim {
    int64_t  sum[3];
    uint64_t windows[3];
    uint32_t valid, reserved;
} mi355x_h264_ssim;
int mi355x_h264_quality_enable_ex(mi355x_h264_encoder *enc, unsigned metrics);
int mi355x_h264_stream_quality_enable_ex(mi355x_h264_stream *s, unsigned metrics);
int64_t mi355x_h264_quality_ssim_read(mi355x_h264_encoder *enc, mi355x_h264_ssim *dst, size_t cap);
int64_t mi355x_h264_quality_ssim_map(mi355x_h264_encoder *enc, int item, int32_t *dst, size_t cap);
int mi355x_h264_stream_last_ssim(const mi355x_h264_stream *s, mi355x_h264_ssim *out);
int64_t mi355x_h264_stream_ssim_map(mi355x_h264_stream *s, int32_t *dst, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
