/*
 * include/mi355x_h264_dec.h -- C ABI of the MI355X H.264 decoder peer.
 *
 * It serves a VideoDecoder peer of the reference's NETINT adapter (interface /root/reference/video_decoder/include/
 * VideoDecoder.h:83, call sites VideoDecoderNetint.cpp: SendStreamData :568, RetrieveFrameData :640): one access unit in,
 * one picture out, output order = decoding order (the streams the reference's encoder side produces have no B pictures).
 *
 * Division of labour: CAVLC slice data is a serial code and is parsed on the host
 * (media_amd/csrc/h264_parse.h); motion compensation, inverse transforms, intra prediction and the loop filter run on the
 * GPU with the encoder's own reconstruction kernels.  No device -> MI355X_H264_E_NODEVICE; there is no CPU reconstruction.
 *
 * Supported: baseline / main / high streams with CAVLC, frame macroblocks, I and P slices, Intra16x16 / Intra4x4 / I_PCM,
 * 16x16 .. 4x4 partitions (every sub_mb_type), up to 3 reference pictures (sliding window, list modification by short-term
 * picture numbers, one index per partition), 4x4 and
 * (inter) 8x8 transform, QP per macroblock
 * (slice_qp_delta, mb_qp_delta), chroma QP index offsets, deblocking filter offsets and idc 0 / 1 / 2 (one set per picture),
 * slices of any shape in raster order (no FMO / ASO).  A stream outside that is refused with MI355X_H264_E_STREAM and a message naming the
 * syntax element; nothing is ever decoded approximately.
 *
 * Many streams on one GPU: mi355x_h264_dec_group_* below decodes the next pictures of up to 64 streams of one coded size in one step.
 */
#ifndef MI355X_H264_DEC_H
#define MI355X_H264_DEC_H

#include <stddef.h>
#include <stdint.h>
#include "mi355x_h264.h"   /* error codes */

#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_H264_E_STREAM (-7)   /* the access unit is damaged or uses a feature outside the supported set (see last_error) */

typedef struct mi355x_h264_decoder mi355x_h264_decoder;

/* replaces ni_device_session_open / ni_logan_decoder_init_default_params (VideoDecoderNetint.cpp:208-262) */
int mi355x_h264_dec_create(int device, mi355x_h264_decoder **out);
void mi355x_h264_dec_destroy(mi355x_h264_decoder *dec);
const char *mi355x_h264_dec_last_error(const mi355x_h264_decoder *dec);

/* one access unit, Annex B with start codes (SendStreamData, VideoDecoderNetint.cpp:568).  *got_picture = 1 when a picture
 * was decoded (0: the unit held parameter sets / SEI only).  The unit is parsed and the picture LAUNCHED on return, not
 * necessarily finished: the next call parses its access unit while the GPU reconstructs this one (one picture of look-ahead).
 * Every call that looks at the picture (read_i420, debug_plane, sync) waits for it first; a failure of the reconstruction
 * itself (MI355X_H264_E_INTERNAL) is reported by that call or by the next decode. */
int mi355x_h264_dec_decode(mi355x_h264_decoder *dec, const uint8_t *au, size_t len, int *got_picture);
/* wait until the picture launched by the last decode call is complete */
int mi355x_h264_dec_sync(mi355x_h264_decoder *dec);

/* cropped and coded size of the last decoded picture (INDEX_PIC_INFO, VideoDecoder.h:57); the native size, whatever output size is set */
int mi355x_h264_dec_picture_info(const mi355x_h264_decoder *dec, int *width, int *height, int *coded_width, int *coded_height);

/* the last decoded picture as tight I420 (Y, U, V planes of the cropped size - never of an output size) into host / device memory; returns bytes or < 0
 * (RetrieveFrameData, VideoDecoderNetint.cpp:640, PIXEL_FORMAT_YUV_420P) */
int64_t mi355x_h264_dec_read_i420(mi355x_h264_decoder *dec, uint8_t *dst, size_t cap);
int64_t mi355x_h264_dec_read_i420_device(mi355x_h264_decoder *dec, void *d_dst, size_t cap);

/* ---- output layouts: the last picture gathered out of the reconstruction ring by ONE kernel (media_amd/csrc/k_dec_out.h) ----
 * Layouts: I420 = Y, U, V planes; NV12 = Y plane, then rows of U, V pairs; NV21 = Y plane, then rows of V, U pairs; RGBA = R, G, B, A
 * bytes, A = 255 (VideoDecoder.h names them PIXEL_FORMAT_YUV_420P, _NV12, _NV21, _RGBA_8888).  RGBA is this build's own definition,
 * integer BT.601 studio swing: c = 298 * (Y - 16), d = U - 128, e = V - 128, R = clip255((c + 409 * e + 128) >> 8),
 * G = clip255((c - 100 * d - 208 * e + 128) >> 8), B = clip255((c + 516 * d + 128) >> 8), the shift arithmetic; the chroma sample
 * of a 2x2 block serves its four pixels.
 * The destination is packed: pictures in stream order, each at an offset rounded up to 256 bytes.  row_align is a power of two
 * 1..256: a luma row, an NV12 / NV21 chroma row and an RGBA row have stride align_up(row bytes, row_align), an I420 chroma row
 * align_up(width / 2, row_align); plane heights are tight; a picture ends with its last row's stride.  Into device memory no byte
 * between a row's end and the next row's start is ever written; into host memory those bytes are unspecified. */
#define MI355X_H264_PIX_I420 0
#define MI355X_H264_PIX_NV12 1
#define MI355X_H264_PIX_NV21 2
#define MI355X_H264_PIX_RGBA 3
typedef struct {
    int64_t offset;                /* of the picture inside the output; -1: the stream has no picture in this output */
    int32_t width, height;         /* size delivered: the cropped size, or the output size set (below, "output size") */
    int32_t stride, chroma_stride; /* bytes per row (chroma_stride: I420 U / V rows, NV12 / NV21 pair rows; 0 for RGBA) */
    int32_t fresh;                 /* 1: decoded in the step the output belongs to */
    int32_t colour;                /* RGBA: matrix | full_range << 8 of the conversion that was applied to the picture (below, "colour"); 0 for
                                    * the other layouts.  (The struct keeps its size: this was a reserved field, always 0.) */
    int64_t serial;                /* that step's serial number (mi355x_h264_dec_group_last_step out[0]; single decoder: pictures decoded) */
} mi355x_h264_dec_out_pic;
/* the last decoded picture in `layout`.  dst == NULL: fills *pic and returns the bytes needed without touching the GPU.  to_device:
 * dst is device memory aligned to 16 bytes, written by a kernel on the decoder's own stream, which waits for no other stream: the
 * caller's work on dst must be complete; the call returns when the picture is there.  Returns the bytes used or < 0 (E_ARG: layout, row_align, cap too small, no picture yet) */
int64_t mi355x_h264_dec_read(mi355x_h264_decoder *dec, int layout, int row_align, void *dst, size_t cap, int to_device,
                             mi355x_h264_dec_out_pic *pic);

/* ---- colour: what the stream says about its samples, and which conversion the RGBA layout applies ----
 * The parser reads the VUI of every sequence parameter set (E.1.1: aspect ratio with Extended_SAR, overscan, video signal type,
 * chroma location, timing, both HRD parameter sets, pic_struct, bitstream restriction).  No field of it is needed to decode samples,
 * so a VUI that is damaged, truncated or out of range NEVER refuses the stream: its fields count as absent, all of them, and the
 * pictures decode as they do without it.
 * mi355x_h264_dec_colour: out[8] for the sequence parameter set the last decoded picture was coded under (E_ARG before the first):
 *   out[0] 1 = a colour description is present, else 0;  out[1] matrix_coefficients, out[2] video_full_range_flag, out[3]
 *   colour_primaries, out[4] transfer_characteristics (2 = unspecified, 0 for the flag, where the stream does not say);
 *   out[5] chroma_sample_loc_type_top_field 0..5, or -1;  out[6] pictures per second, time_scale / (2 * num_units_in_tick) rounded,
 *   or 0;  out[7] max_num_reorder_frames, or -1 (0: every picture may be handed out as soon as it is decoded).
 * RGBA output applies the variant the stream describes - the four sets of mi355x_h264.h, "colour description" - when its
 * matrix_coefficients are 1 (BT.709), 5 or 6 (both: the BT.601 numbers), with the range its video_full_range_flag names.  Every
 * other stream, one without a description included, gets BT.601 limited as stated above.  A group's launch serves streams of
 * different descriptions at once: the variant belongs to the picture, not to the launch.
 * mi355x_h264_dec_set_rgba_colour overrides that for the handle's (the group form: the stream's) pictures from the next read or armed
 * step on, whatever the stream says; NULL: follow the stream again.  E_ARG: a matrix other than MI355X_H264_MATRIX_BT709 / _BT601,
 * full_range outside 0 / 1, a wrong struct_size, no such stream.
 * mi355x_h264_dec_out_pic.colour names the variant that WAS applied: MI355X_H264_MATRIX_* | full_range << 8 (a stream that says 5 is
 * reported as 6, whose numbers it got). */
int mi355x_h264_dec_colour(const mi355x_h264_decoder *dec, int32_t out[8]);
int mi355x_h264_dec_set_rgba_colour(mi355x_h264_decoder *dec, const mi355x_h264_colour *colour);

/* ---- decoder groups: the next pictures of up to 64 streams reconstructed in ONE step ----
 * One decoder object per stream costs each picture its own uploads and five to eight launches that fill a fraction of the GPU.  A
 * group decodes the streams' next access units together: they are parsed side by side on a small pool of threads the group owns
 * (min(streams, 8); MI355X_H264_DEC_PARSE_THREADS = 1..16), and the step then makes one set of transfers and one set of launches
 * whatever the number of streams.  All streams of a group have one coded size - that of the first IDR picture any of them delivers;
 * a stream of another size is refused with E_STREAM, the others go on.  Every stream keeps what a decoder keeps: its parser, its
 * reference pictures and ring position, its crop, and the rule that after an error P pictures are refused until its next IDR
 * picture.  A damaged or unsupported access unit fails its own stream only.  A group is driven by one thread at a time. */
typedef struct mi355x_h264_dec_group mi355x_h264_dec_group;
int mi355x_h264_dec_group_create(int device, int streams /* 1..64 */, mi355x_h264_dec_group **out);
void mi355x_h264_dec_group_destroy(mi355x_h264_dec_group *g);
/* one STEP: aus[i] / lens[i] = the next access unit of stream i, or aus[i] = NULL: stream i takes no part in this step.
 * rc[i] = MI355X_H264_OK / E_STREAM / ... per stream, got[i] = 1 when stream i decoded a picture in this step (all four arrays have
 * `streams` entries).  Returns < 0 only for what concerns the whole group (arguments, device, a timed-out wavefront - which leaves
 * every picture of its step unusable as a reference: all its streams wait for an IDR picture).  The step is LAUNCHED on return, not
 * necessarily finished: the next call parses while the GPU reconstructs, and waits for the step in flight before it launches its
 * own.  read_*, debug_plane and sync wait first.  MI355X_H264_DEC_SYNC=1 waits inside every call, as for the single decoder. */
int mi355x_h264_dec_group_decode(mi355x_h264_dec_group *g, const uint8_t *const *aus, const size_t *lens, int *got, int *rc);
int mi355x_h264_dec_group_sync(mi355x_h264_dec_group *g);
/* the message of stream's last refusal; stream = -1: of the group's own last failure */
const char *mi355x_h264_dec_group_last_error(const mi355x_h264_dec_group *g, int stream);
/* the stream's last decoded picture: as the single decoder's calls of these names */
int mi355x_h264_dec_group_picture_info(const mi355x_h264_dec_group *g, int stream, int *w, int *h, int *cw, int *ch);
int mi355x_h264_dec_group_colour(const mi355x_h264_dec_group *g, int stream, int32_t out[8]);
int mi355x_h264_dec_group_set_rgba_colour(mi355x_h264_dec_group *g, int stream, const mi355x_h264_colour *colour);
int64_t mi355x_h264_dec_group_read_i420(mi355x_h264_dec_group *g, int stream, uint8_t *dst, size_t cap);
int64_t mi355x_h264_dec_group_read_i420_device(mi355x_h264_dec_group *g, int stream, void *d_dst, size_t cap);
int64_t mi355x_h264_dec_group_debug_plane(mi355x_h264_dec_group *g, int stream, int plane, void *dst, size_t cap);
/* what the last step was: out[0] its serial number, out[1] pictures it carried, out[2] kernel launches it made, out[3] host-to-device
 * transfers it made, out[4] parse threads used; with n >= 7 also out[5] / out[6]: microseconds the host spent parsing / launching
 * (and, with MI355X_H264_DEC_SYNC, waiting); with n >= 9 also out[7] / out[8]: output launches / device-to-host output transfers the
 * step made (set_output below; 0 / 0 for an unarmed group); with n >= 11 also out[9] / out[10]: launches / transfers of the last
 * read_all call; with n >= 13 also out[11] / out[12]: bytes of device memory / of pinned host memory the group holds at the moment
 * of the call (its picture store and its own arrays, tables and output buffers; not the parsers' heap).  Returns the number of
 * values written */
int mi355x_h264_dec_group_last_step(const mi355x_h264_dec_group *g, int64_t *out, int n);

/* every stream's last decoded picture in ONE call (layouts and packing: above): what read_i420 gives per stream, for all streams
 * that have a picture, in stream order.  pics[streams] is filled: offset -1 for a stream without a picture; fresh = 1 for a stream
 * that decoded in the last step, 0 for one that sat it out or was refused; serial = the last step's.  dst == NULL: sizes only
 * (fills pics, returns the bytes needed, does not touch the GPU).  Waits for the step in flight, then makes one launch - straight into
 * dst when to_device (device memory aligned to 16 bytes; no transfer), else into a device staging buffer followed by ONE
 * device-to-host copy through a pinned buffer and a host copy to dst - whatever the number of streams.  The position table lies in
 * pinned memory that the kernel reads in place.  Returns the bytes used or < 0 (E_ARG: layout, row_align, cap too small, no stream
 * has a picture) */
int64_t mi355x_h264_dec_group_read_all(mi355x_h264_dec_group *g, int layout, int row_align, void *dst, size_t cap, int to_device,
                                       mi355x_h264_dec_out_pic *pics /* [streams] */);
/* arm the group (layout -1: disarm): from the next step on every step that carries pictures is followed, on the group's one stream
 * behind the loop filter, by one gather launch for exactly the step's positions and one asynchronous device-to-host copy into one
 * of two pinned output sets, with an event of its own.  The sets take turns.  The step's table of output positions travels behind
 * its position table in the same transfer: out[2] / out[3] of last_step count what they count for an unarmed group. */
int mi355x_h264_dec_group_set_output(mi355x_h264_dec_group *g, int layout, int row_align);
/* the output of an armed step.  back = 0: of the last step that carried pictures - waits for that step's event and reports a
 * wavefront time-out of the step as sync does; back = 1: of the one before it, which is complete: never waits on the GPU.  *data
 * points into the pinned set and stays valid until the second decode call after the step; pics[streams]: offset -1 for the streams
 * that took no part in that step.  E_ARG: unarmed, or fewer than back + 1 armed steps so far */
int mi355x_h264_dec_group_output(mi355x_h264_dec_group *g, int back, const uint8_t **data, mi355x_h264_dec_out_pic *pics);

/* ---- output size: pictures resampled on the GPU to a requested size (media_amd/csrc/k_dec_out_scale.h) ----
 * A decoder, or a stream of a group, may have an output size (W, H).  The picture delivered in layout L is then exactly what the
 * unscaled call delivers in L, with the same row_align and the same colour variant, for a decoded picture whose cropped I420 planes
 * are the area-resampled planes: Y resampled from the cropped size (w, h) to (W, H), Cb and Cr each from (w / 2, h / 2) to
 * (W / 2, H / 2).  The arithmetic is that of mi355x_h264.h, "scaled streams": integer overlap weights, and one exact division
 * floor((N + (D >> 1)) / D) per sample; nothing is rounded between the horizontal and the vertical sums.  RGBA resamples the three
 * planes first and converts then: the chroma sample of a 2x2 block of the RESULT serves its four pixels.  A dimension with W == w is
 * the identity by this arithmetic.
 * set_output_size: (0, 0) = the native size again; stream = -1: every stream of the group.  E_ARG, before the device is touched: an
 * odd value, a value outside 2..4096, exactly one of the two values 0, no such stream.  The setting holds from the next dec_read /
 * read_all call and from the next armed step on; the same picture may be read again and again at different sizes (a rendition
 * ladder from one decode).  Output buffers sized for the native picture always suffice.
 * Whether a picture can be resampled is checked when it is delivered: W <= w <= 4 W and H <= h <= 4 H must hold (no upscaling, no
 * ratio above 4).  Otherwise dec_read returns E_ARG and last_error names both sizes; in read_all and in an armed step that stream's
 * pics[i].offset is -1 and mi355x_h264_dec_group_last_error(g, i) says why, while the other streams are delivered (read_all: E_ARG
 * when no stream is deliverable, as for "no stream has a picture").
 * mi355x_h264_dec_out_pic.width / height / stride / chroma_stride describe the picture DELIVERED, and dst == NULL sizing follows
 * them.  A call none of whose streams has an output size makes the launch it always made; a call with at least one makes ONE launch
 * of the resampling kernel for all its pictures (the others pass through ratio 1), and the transfers the unscaled call makes.
 * Left at the native size: _picture_info, _read_i420(_device), _group_read_i420(_device), debug_plane. */
int mi355x_h264_dec_set_output_size(mi355x_h264_decoder *dec, int width, int height);
int mi355x_h264_dec_output_size(const mi355x_h264_decoder *dec, int *width, int *height);
int mi355x_h264_dec_group_set_output_size(mi355x_h264_dec_group *g, int stream, int width, int height);
int mi355x_h264_dec_group_output_size(const mi355x_h264_dec_group *g, int stream, int *width, int *height);

/* ---- loss mode: conceal lost slices and pictures, join at a recovery point, and know when pictures are exact again ----
 * A decoder, or a stream of a group, has a loss mode.  MI355X_H264_LOSS_STRICT (0, the default) is everything said above: a picture
 * whose slices leave a hole, a frame_num that does not follow, a P picture with nothing held are refused, and the stream waits for an
 * IDR picture.  MI355X_H264_LOSS_CONCEAL (1) decodes on.  The mode may be set at any time between calls; E_ARG for another mode, no
 * such stream, a null handle.  Strict and concealing streams share a group and its steps; a stream left strict keeps every refusal,
 * message, launch, copy and allocation it had.
 *
 * Concealment is not normative; this is the library's definition: WHAT IS MISSING IS DECODED AS IF AN ALL-P_SKIP SLICE HAD ARRIVED IN
 * ITS PLACE, so that any conforming decoder fed the stream with those slices put in produces the same samples.
 *   Missing or damaged slice.  A hole in the macroblock addresses - from the address behind the last received slice (0 at the start
 *   of the picture) to the next received slice's first_mb_in_slice, or to the end of the picture - is filled.  A slice NAL unit that
 *   does not parse, in its header or anywhere in its data, is dropped WHOLE and its extent becomes such a hole (so does a slice that
 *   runs on into the next one).  The fill stands for ONE P slice of exactly those macroblocks: one mb_skip_run; the picture parameter
 *   set, reference list and deblocking parameters of the picture's received slices; slice QP = that of the preceding slice in
 *   decoding order (the last slice of the previous picture if the hole comes first; pic_init_qp if there is no previous picture).  By
 *   8.4.1.1 every vector of such a slice is (0, 0) with ref_idx 0: a copy from the newest reference picture, loop-filtered or not
 *   exactly as the standard says for that slice.  The host writes the per-macroblock arrays for those macroblocks and they go through
 *   the step's ordinary launches: a partly received picture costs no launch.  An access unit with slices none of which is usable
 *   yields got_picture = 0 and counts as a lost picture; so does an IDR picture with a hole (a P slice cannot stand in one).  A slice
 *   that names a parameter set the stream has not delivered, and whatever is wrong outside slice NAL units, is refused as in strict
 *   mode; a refused stream joins again (below) with its next picture.
 *   Missing reference pictures.  g = (frame_num - PrevRefFrameNum - 1) mod MaxFrameNum > 0: each of the g missing pictures stands for
 *   an all-skip picture, a copy of the newest held picture.  Nothing is output for them and no step is run: the reference list entry of
 *   age a (the missing pictures counted) means the held picture of real age max(0, a - g), and min(held + g, max_num_ref_frames)
 *   pictures are held afterwards.  A P picture behind a lost IDR picture falls under the same rule; lost non-reference pictures leave
 *   no gap.
 *   Joining.  A concealing stream that holds parameter sets (fed as an access unit of SPS + PPS, which decode accepts with
 *   got_picture = 0) and no reference picture decodes a picture that is no IDR picture against reference pictures whose samples are
 *   all 128, Y, U and V, and holds max_num_ref_frames of them.  A group without a coded size takes that picture's.  The grey pictures
 *   are written by one store-only launch (media_amd/csrc/k_dec_ring.h) per step for all its joining streams, ahead of reconstruction:
 *   mi355x_h264_dec_group_last_step out[2] is one higher in such a step and in no other.
 *
 * The damage map: a byte per macroblock of the last picture, raster order; bit 0 TAINTED = its samples may differ from the lossless
 * decode, bit 1 CONCEALED = it was filled in in this picture.  The rules are conservative (a clean macroblock IS exact; a tainted one
 * may be) and work on whole macroblocks (media_amd/csrc/dec_loss.h):
 *   a concealed macroblock is tainted; every macroblock of a grey or stand-in picture is tainted; I_PCM is clean;
 *   an inter partition taints its macroblock if a tainted macroblock of the picture it refers to overlaps the rectangle it reads -
 *   the block plus the six-tap margins (2 before, 3 behind) where the vector component is fractional (8.4.2.2.1), the chroma block
 *   plus one sample where it has a fraction (8.4.2.2.2), clamped to the picture;
 *   an intra macroblock is tainted if a neighbour A, B, C or D that its prediction may read - in its slice, and intra where
 *   constrained_intra_pred_flag says so - is tainted;
 *   then, in decoding order, a filtered left or top macroblock edge taints both its macroblocks if either is tainted:
 *   disable_deblocking_filter_idc 1 filters none, 2 none across a slice edge;
 *   an IDR picture whose slices were all received is therefore clean.
 * mi355x_h264_dec_damage out[6]: [0] tainted macroblocks of the last picture (0: it is exact), [1] macroblocks concealed in it, [2]
 * reference pictures stood in for before it (g), [3] recovery_frame_cnt of a recovery point SEI (payload type 6) in its access unit,
 * else -1 (read in both modes; a damaged SEI never refuses a stream), [4] pictures decoded since the stream's last loss, join or
 * refusal (the picture of the loss counts 0), [5] 1 = the stream joined without an IDR picture and has not been clean since.
 * mi355x_h264_dec_damage_map: the map into dst[cap], returns its bytes (E_ARG: no picture yet, cap too small).  A strict stream
 * reports a clean picture.  One exception keeps the report sound across a change of mode: a stream that has decoded in conceal mode
 * keeps its maps going after it is set to strict again (its reference pictures may still be tainted), and both calls go on reporting
 * them, until its group's coded size changes.  An access unit with more than 32 damaged slices is refused as in strict mode. */
#define MI355X_H264_LOSS_STRICT 0
#define MI355X_H264_LOSS_CONCEAL 1
int mi355x_h264_dec_set_loss_mode(mi355x_h264_decoder *dec, int mode);
int mi355x_h264_dec_damage(const mi355x_h264_decoder *dec, int32_t out[6]);
int64_t mi355x_h264_dec_damage_map(const mi355x_h264_decoder *dec, uint8_t *dst, size_t cap);
int mi355x_h264_dec_group_set_loss_mode(mi355x_h264_dec_group *g, int stream, int mode);
int mi355x_h264_dec_group_damage(const mi355x_h264_dec_group *g, int stream, int32_t out[6]);
int64_t mi355x_h264_dec_group_damage_map(const mi355x_h264_dec_group *g, int stream, uint8_t *dst, size_t cap);

/* ---- test / measurement hooks ---- */
int64_t mi355x_h264_dec_debug_plane(mi355x_h264_decoder *dec, int plane, void *dst, size_t cap);   /* coded-size plane 0..2 (never resampled) */
int mi355x_h264_dec_timing(const mi355x_h264_decoder *dec, uint64_t *pictures, double *parse_ms, double *gpu_ms);
/* mi355x_h264_dec_group_last_step of the group of one stream that the decoder is */
int mi355x_h264_dec_last_step(const mi355x_h264_decoder *dec, int64_t *out, int n);

/* Guard mode of the library's own memory (mi355x_h264.h, mi355x_h264_debug_mem_guard: the switch and the tally are process-wide and
 * hold for decoders and groups created afterwards).  Off (the default): no launch, no copy and no allocation differs.  The check
 * waits as mi355x_h264_dec_group_sync does (and for an armed step's copy), then compares the guards of the picture store's blocks
 * and the group's own, and the ring's zeroed slack; return value, *regions, report and the poke's arguments as for the encoder.  A
 * decoder's check is its group's.  Blocks that are dropped and made again (the lists of large levels, output staging, a decoder's
 * change of coded size) are checked as they are freed: mi355x_h264_debug_mem_tally. */
int mi355x_h264_dec_debug_mem_check(mi355x_h264_decoder *dec, int *regions, char *report, size_t cap);
int mi355x_h264_dec_group_debug_mem_check(mi355x_h264_dec_group *g, int *regions, char *report, size_t cap);
int mi355x_h264_dec_group_debug_mem_poke(mi355x_h264_dec_group *g, const char *block, int64_t offset, int value);

/* the host parser alone (needs no GPU): parse one access unit and read back what it recovered */
typedef struct mi355x_h264_parser mi355x_h264_parser;
mi355x_h264_parser *mi355x_h264_parser_create(void);
void mi355x_h264_parser_destroy(mi355x_h264_parser *p);
int mi355x_h264_parser_parse(mi355x_h264_parser *p, const uint8_t *au, size_t len);   /* 1 picture, 0 none, -1 error */
const char *mi355x_h264_parser_error(const mi355x_h264_parser *p);
/* out[12]: mbw, mbh, width, height, idr, qp (of the first slice), slice_rows (0 = one slice, n > 0 = bands of n rows, -1 = slices
 * of any other shape), deblocking idc, num_ref_idx_active,
 * transform_8x8_mode, has I_PCM, bit 0 has intra | bit 1 has inter; with n >= 17 also: chroma_qp_index_offset,
 * second_chroma_qp_index_offset, FilterOffsetA, FilterOffsetB, 1 = every macroblock has that one QP and no offset applies;
 * with n >= 20 also RefPicList0 entries 0..2 as "reference pictures ago" (0 = the one decoded last; default 0, 1, 2);
 * with n >= 21 also 1 = a reference picture (nal_ref_idc != 0), 0 = a non-reference picture.
 * Returns the number of values written */
int mi355x_h264_parser_info(const mi355x_h264_parser *p, int32_t *out, int n);
/* what: 0 MbInfo (32 B / macroblock, layout of mi355x_h264.h), 1 quadrant vectors (8 int16), 2 Intra4x4 modes (16 B), 3 levels (416 int16),
 * 4 QP_Y (1 B / macroblock; 0 for I_PCM), 5 vectors per 4x4 block (32 int16, raster order), 6 ref_idx_l0 per 8x8 quadrant (4 B; 255 intra),
 * 7 neighbour availability (1 B: bits 0..3 the left, above, above-right, above-left macroblock lies in this slice and was decoded
 *   before; bits 4..7 it may also be used for intra prediction: constrained_intra_pred_flag) */
int64_t mi355x_h264_parser_read(const mi355x_h264_parser *p, int what, void *dst, size_t cap);
/* the parser's half of the loss mode (above): in MI355X_H264_LOSS_CONCEAL parse fills holes, takes frame_num gaps and joins in;
 * parser_read what = 8 then gives 1 B / macroblock, 1 = filled in.  parser_loss out[5] for the last access unit: macroblocks filled in,
 * g, 1 = the picture joined, recovery_frame_cnt or -1 (both modes), 1 = it held slices but no usable picture (parse returned 0) */
int mi355x_h264_parser_set_loss_mode(mi355x_h264_parser *p, int mode);
int mi355x_h264_parser_loss(const mi355x_h264_parser *p, int32_t out[5]);
/* out[8] of mi355x_h264_dec_colour for the sequence parameter set the last slice referred to (before the first: set 0, absent
 * fields); with n >= 10 also out[8] 1 = the set has a VUI that was read whole and in range, out[9] max_dec_frame_buffering or -1.
 * Returns the number of values written, or -1 */
int mi355x_h264_parser_colour(const mi355x_h264_parser *p, int32_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif
