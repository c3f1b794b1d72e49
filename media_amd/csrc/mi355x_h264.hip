// media_amd/csrc/mi355x_h264.hip -- the C ABI of include/mi355x_h264.h and include/mi355x_h264_dec.h.  The library is this ONE
// translation unit: the kernels (k_*.h, rgba_kernels.h), host_framing.h (parameter sets, slice header, NAL escaping, tables; no
// HIP), pic_store.h (what encoder and decoder share: ring, per-macroblock arrays, flags), engine.h (mi355x_h264_encoder),
// hub_sched.h + hub.h (the stream hub: scheduling without HIP, device side; damage.h + k_patch.h: its damage tiles), dec_group.h
// (decoder groups) and decoder.h (the decoder peer: a group of one stream).  Every entry point below checks its arguments and
// calls into one of them.  There is no CPU encode path:
// without a HIP device create() fails.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/mi355x_h264.h"
#include "dev_common.h"
#include "k_cavlc.h"
#include "k_deblock.h"
#include "k_intra.h"
#include "k_me.h"
#include "k_tq.h"
#include "k_dec.h"
#include "k_dec_ring.h"
#include "k_quality.h"
#include "h264_parse.h"
#include "../../include/mi355x_h264_dec.h"

using namespace h264;

#include "host_framing.h"
#include "rgba_kernels.h"
#include "scale_kernels.h"
#include "damage.h"
#include "k_patch.h"
#include "k_dec_out.h"
#include "k_dec_out_scale.h"
#include "dev_mem.h"
#include "pic_store.h"
#include "engine.h"
#include "hub_sched.h"
#include "hub.h"
#include "dec_group.h"
#include "decoder.h"

extern "C" {

int mi355x_h264_abi_version(void) { return MI355X_H264_ABI_VERSION; }

void mi355x_h264_default_config(mi355x_h264_config* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->struct_size = sizeof(*c);
    c->width = 720; c->height = 1280;  // reference defaults, VideoEncoderOpenH264.h:13-24
    c->fps = 30; c->bitrate = 5000000; c->gop = 30; c->profile_idc = 66;
    c->rc_mode = MI355X_H264_RC_FIXED_QP; c->qp = 26; c->device = 0; c->disable_deblock = 0;
    c->search = MI355X_H264_SEARCH_SEEDED;
}

int mi355x_h264_create(const mi355x_h264_config* cfg, mi355x_h264_encoder** out) { return create_engine(cfg, out, false); }

// a caller's description as the owners keep it; false: refused (matrix, range or struct_size)
static bool colour_take(const mi355x_h264_colour* c, ColourDesc* d)
{
    *d = ColourDesc();
    if (!c) return true;
    if (c->struct_size != sizeof(mi355x_h264_colour) || !colour_valid(c->matrix, c->full_range)) return false;
    d->described = 1; d->matrix = c->matrix; d->full_range = c->full_range;
    return true;
}
static int colour_give(const ColourDesc& d, mi355x_h264_colour* out)
{
    out->struct_size = sizeof(*out); out->matrix = d.described ? d.matrix : MI355X_H264_MATRIX_BT601; out->full_range = d.described ? d.full_range : 0;
    return d.described;
}

int mi355x_h264_create_colour(const mi355x_h264_config* cfg, const mi355x_h264_colour* colour, mi355x_h264_encoder** out)
{
    ColourDesc d;
    if (out) *out = nullptr;
    if (!colour_take(colour, &d)) return MI355X_H264_E_ARG;
    return create_engine(cfg, out, false, &d, false);
}
int mi355x_h264_colour_of(const mi355x_h264_encoder* e, mi355x_h264_colour* out) { return e && out ? colour_give(e->colour, out) : MI355X_H264_E_ARG; }
void mi355x_h264_destroy(mi355x_h264_encoder* e) { destroy_engine(e); }

#define NEED(e, cond, what) do { if (!(e)) return MI355X_H264_E_ARG; if (!(cond)) return set_err((e)->err, MI355X_H264_E_ARG, what); } while (0)

int mi355x_h264_encode_device(mi355x_h264_encoder* e, const void* d_pic, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, d_pic && out && out_len, "null argument");
    return encode_one_device(e, d_pic, e->cfg.input_format == MI355X_H264_INPUT_NV12, out, out_len, frame_type);
}

int mi355x_h264_encode(mi355x_h264_encoder* e, const uint8_t* y, int ys, const uint8_t* u, int us, const uint8_t* v, int vs,
                       uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, y && u && v && out && out_len, "null argument");
    const int w = e->cfg.width;
    NEED(e, ys >= w && us >= w / 2 && vs >= w / 2, "stride smaller than width");
    return encode_one_host(e, HostPicture{PIC_I420, {y, u, v}, {ys, us, vs}}, 4, out, out_len, frame_type);
}

int mi355x_h264_encode_nv12_device(mi355x_h264_encoder* e, const void* d_nv12, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, d_nv12 && out && out_len, "null argument");
    return encode_one_device(e, d_nv12, true, out, out_len, frame_type);   // the kernels read the interleaved chroma themselves
}

int mi355x_h264_encode_nv12(mi355x_h264_encoder* e, const uint8_t* y, int ys, const uint8_t* uv, int uvs, uint8_t** out,
                            uint32_t* out_len, int* frame_type)
{
    NEED(e, y && uv && out && out_len, "null argument");
    NEED(e, ys >= e->cfg.width && uvs >= e->cfg.width, "stride smaller than width");
    return encode_one_host(e, HostPicture{PIC_NV12, {y, uv, nullptr}, {ys, uvs, 0}}, 1, out, out_len, frame_type);
}

int mi355x_h264_encode_rgba_device(mi355x_h264_encoder* e, const void* d_rgba, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, d_rgba && out && out_len, "null argument");
    NEED(e, e->G == 1, "single-picture calls need a batch-1 encoder");
    NEED(e, ((uintptr_t)d_rgba & 7) == 0, "RGBA picture not aligned to 8 bytes");
    HIPCHK(e->err, hipSetDevice(e->device));
    return encode_rgba_from_device(e, (const uint8_t*)d_rgba, (size_t)e->cfg.width * 4, out, out_len, frame_type);
}

int mi355x_h264_encode_rgba(mi355x_h264_encoder* e, const uint8_t* rgba, int stride, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, rgba && out && out_len, "null argument");
    NEED(e, e->G == 1, "single-picture calls need a batch-1 encoder");
    const int w = e->cfg.width, h = e->cfg.height;
    NEED(e, stride >= 4 * w, "stride smaller than 4 * width");
    HIPCHK(e->err, hipSetDevice(e->device));
    const size_t n = picture_bytes(PIC_RGBA, w, h);
    if (!DM_PAIR(e->mem, e->d_rgba, e->h_rgba, n + 256))   // staging for RGBA pictures: comes with the first one
        return set_err(e->err, MI355X_H264_E_NOMEM, "no memory for the RGBA staging picture");
    HIPCHK(e->err, stage_picture(HostPicture{PIC_RGBA, {rgba, nullptr, nullptr}, {stride, 0, 0}}, w, h, e->h_rgba, e->d_rgba, e->stream, 1));
    return encode_rgba_from_device(e, e->d_rgba, (size_t)w * 4, out, out_len, frame_type);
}

int mi355x_h264_encode_batch_device(mi355x_h264_encoder* e, const void* d_frames, size_t stride, int count, uint8_t* host_out,
                                    size_t out_cap, uint32_t* sizes, size_t* total_len)
{
    NEED(e, d_frames && host_out && sizes && count >= 0, "null argument");
    NEED(e, e->G == 1, "use mi355x_h264_encode_gops_device with a batched encoder");
    HIPCHK(e->err, hipSetDevice(e->device));
    const bool nv12 = e->cfg.input_format == MI355X_H264_INPUT_NV12;
    size_t pos = 0;
    quality_begin(e, (size_t)count, 0, 0);
    const int rc = run_pipeline(e, count,
        [&](int i, int slot) { return submit(e, (const uint8_t*)d_frames + (size_t)i * stride, 0, slot, nv12); },
        [&](int i, int slot) -> int {
            uint8_t* p = nullptr; uint32_t n = 0;
            e->q_add = (size_t)i;
            const int r = collect(e, slot, &p, &n, nullptr);
            if (r) return r;
            if (pos + n > out_cap) {
                e->seq.force_idr = 1;   // this picture (and those in flight behind it) never reach the caller: the next one must not refer to them
                return set_err(e->err, MI355X_H264_E_OVERFLOW, "batch output buffer too small");
            }
            memcpy(host_out + pos, p, n);
            sizes[i] = n;
            pos += n;
            return 0;
        });
    if (rc) return rc;
    if (total_len) *total_len = pos;
    return MI355X_H264_OK;
}

int mi355x_h264_encode_gops_device(mi355x_h264_encoder* e, const void* d_frames, size_t frame_stride, size_t gop_stride, int frames_per_gop,
                                   uint8_t* host_out, size_t out_cap_per_gop, uint32_t* sizes, size_t* gop_bytes)
{
    NEED(e, d_frames && host_out && sizes && gop_bytes && frames_per_gop >= 1, "null argument");
    HIPCHK(e->err, hipSetDevice(e->device));
    const int G = e->G;
    const bool nv12 = e->cfg.input_format == MI355X_H264_INPUT_NV12;
    for (int g = 0; g < G; g++) gop_bytes[g] = 0;
    e->seq.force_idr = 1;                     // every call starts closed GOPs
    quality_begin(e, (size_t)G * frames_per_gop, (size_t)frames_per_gop, 0);
    return run_pipeline(e, frames_per_gop,
        [&](int i, int slot) { return submit(e, (const uint8_t*)d_frames + (size_t)i * frame_stride, gop_stride, slot, nv12); },
        [&](int i, int slot) -> int {
            e->q_add = (size_t)i;
            int r = wait_slot(e, slot);
            for (int g = 0; g < G && !r; g++) {
                uint8_t* p = nullptr; uint32_t n = 0;
                r = finish_item(e, e->slots[slot], e->slots[slot].lay, e->slots[slot].pics[g], &p, &n, nullptr);
                if (r) break;
                if (gop_bytes[g] + n > out_cap_per_gop) return set_err(e->err, MI355X_H264_E_OVERFLOW, "gop output buffer too small");
                memcpy(host_out + (size_t)g * out_cap_per_gop + gop_bytes[g], p, n);
                sizes[(size_t)g * frames_per_gop + i] = n;
                gop_bytes[g] += n;
            }
            return r;
        });
}

int mi355x_h264_force_idr(mi355x_h264_encoder* e) { if (!e) return MI355X_H264_E_ARG; e->seq.force_idr = 1; return MI355X_H264_OK; }

int mi355x_h264_last_me_cost(const mi355x_h264_encoder* e, uint32_t* cost)
{
    if (!e || !cost) return MI355X_H264_E_ARG;
    for (int g = 0; g < e->G; g++) cost[g] = e->last_me_cost[g];
    return MI355X_H264_OK;
}

int mi355x_h264_set_qp(mi355x_h264_encoder* e, int qp) { if (!e || qp < 10 || qp > 51) return MI355X_H264_E_ARG; e->qp = qp; return MI355X_H264_OK; }

// ---- temporal layers (host_framing.h, PicSeq; k_me.h) ----
int mi355x_h264_set_temporal_layers(mi355x_h264_encoder* e, int layers)
{
    NEED(e, layers == 1 || layers == 2, "temporal layers: 1 or 2");
    NEED(e, layers == 1 || e->cfg.band_count <= 1, "temporal layers: not on a band instance (the halo exchange is the caller's)");
    NEED(e, layers == 1 || !e->shape.refresh, "temporal layers: not with intra refresh");
    NEED(e, e->seq.frames == 0, "temporal layers: before the first picture only");
    e->seq.layers = layers;
    return MI355X_H264_OK;
}
int mi355x_h264_last_temporal_id(const mi355x_h264_encoder* e) { return e ? e->last_layer : MI355X_H264_E_ARG; }
int mi355x_h264_stream_last_temporal_id(const mi355x_h264_stream* s) { return s ? s->hub->sched.last_layer(s->item) : MI355X_H264_E_ARG; }

// ---- intra refresh (host_framing.h, PicSeq::refresh_band; k_me.h, the RFR form) ----
int mi355x_h264_set_intra_refresh(mi355x_h264_encoder* e, int on)
{
    NEED(e, on == 0 || on == 1, "intra refresh: 0 or 1");
    NEED(e, e->seq.frames == 0, "intra refresh: before the first picture only");
    if (on) {
        NEED(e, e->cfg.slices >= 2 && e->cfg.slices <= 32, "intra refresh: an encoder with slices = 2 .. 32");
        NEED(e, refresh_bands(e->mbh, e->cfg.slices) == e->cfg.slices, "intra refresh: the picture does not divide into that many bands of two rows or more");
        NEED(e, e->cfg.refs <= 1, "intra refresh: one reference picture");
        NEED(e, e->seq.layers == 1, "intra refresh: one temporal layer");
        NEED(e, e->cfg.band_count <= 1, "intra refresh: not on a band instance");
    }
    e->shape.refresh = on;
    e->seq.refresh_n = on ? e->nsl : 0;
    return MI355X_H264_OK;
}
int mi355x_h264_last_refresh_band(const mi355x_h264_encoder* e) { return e ? e->last_rband[0] : MI355X_H264_E_ARG; }
int mi355x_h264_stream_last_refresh_band(const mi355x_h264_stream* s) { return s ? s->hub->sched.last_rband(s->item) : MI355X_H264_E_ARG; }

int mi355x_h264_set_idr_pic_id(mi355x_h264_encoder* e, int next, int step)
{
    if (!e) return MI355X_H264_E_ARG;
    e->seq.idr_id = next & 0xFF; e->idr_step = step;
    return MI355X_H264_OK;
}

int mi355x_h264_band_info(const mi355x_h264_encoder* e, int* first_row, int* rows, int* first_slice, int* slices, size_t* halo_bytes)
{
    if (!e) return MI355X_H264_E_ARG;
    if (first_row) *first_row = e->b_row0;
    if (rows) *rows = e->b_rows;
    if (first_slice) *first_slice = e->b_sl0;
    if (slices) *slices = e->b_nsl;
    if (halo_bytes) *halo_bytes = (size_t)HALO_MB_ROWS * 16 * e->cw * 3 / 2;
    return MI355X_H264_OK;
}

int mi355x_h264_band_halo_export(mi355x_h264_encoder* e, int edge, void* d_dst)
{
    NEED(e, d_dst && (edge == 0 || edge == 1), "bad argument");
    HIPCHK(e->err, hipSetDevice(e->device));
    const int n = std::min((int)HALO_MB_ROWS, e->b_rows);
    const int r0 = edge == 0 ? e->b_row0 : e->b_row0 + e->b_rows - n;
    return halo_copy(e, r0, r0 + n, d_dst, true);
}

int mi355x_h264_band_halo_import(mi355x_h264_encoder* e, int edge, const void* d_src)
{
    NEED(e, d_src && (edge == 0 || edge == 1), "bad argument");
    HIPCHK(e->err, hipSetDevice(e->device));
    // above: the neighbour's LAST rows end right above this band; below: its FIRST rows start right below
    int r0, r1;
    if (edge == 0) { r1 = e->b_row0; r0 = std::max(0, r1 - (int)HALO_MB_ROWS); if (r1 - r0 < (int)HALO_MB_ROWS && r1 > 0) return set_err(e->err, MI355X_H264_E_INTERNAL, "band above is shorter than the halo"); }
    else { r0 = e->b_row0 + e->b_rows; r1 = std::min(e->mbh, r0 + (int)HALO_MB_ROWS); }
    if (r1 <= r0) return MI355X_H264_OK;   // picture edge: nothing beyond
    return halo_copy(e, r0, r1, const_cast<void*>(d_src), false);
}

const char* mi355x_h264_last_error(const mi355x_h264_encoder* e) { return e ? e->err : "null encoder"; }
int mi355x_h264_coded_width(const mi355x_h264_encoder* e) { return e ? e->cw : 0; }
int mi355x_h264_coded_height(const mi355x_h264_encoder* e) { return e ? e->ch : 0; }

int mi355x_h264_debug_keep_pre(mi355x_h264_encoder* e, int on) { if (!e) return MI355X_H264_E_ARG; e->keep_pre = on != 0; return MI355X_H264_OK; }

int64_t mi355x_h264_debug_read(mi355x_h264_encoder* e, int what, void* dst, size_t cap)
{
    if (!e || !dst) return MI355X_H264_E_ARG;
    if (hipSetDevice(e->device) != hipSuccess) return MI355X_H264_E_HIP;
    const void* src = nullptr;
    size_t n = 0;
    const size_t ysz = (size_t)e->cw * e->ch;
    const int last = e->seq.last_slot(e->nbuf);  // picture finished by the last encode (a layer-1 picture leaves seq.cur where it was)
    switch (what) {
        case MI355X_H264_DBG_RECON_Y: case MI355X_H264_DBG_RECON_U: case MI355X_H264_DBG_RECON_V:
            src = e->d_planes[last][what]; n = what ? ysz / 4 : ysz; break;
        case MI355X_H264_DBG_PRE_Y: case MI355X_H264_DBG_PRE_U: case MI355X_H264_DBG_PRE_V:
            src = e->d_pre[what - MI355X_H264_DBG_PRE_Y]; n = what != MI355X_H264_DBG_PRE_Y ? ysz / 4 : ysz; break;
        case MI355X_H264_DBG_MBINFO: src = e->d_mb; n = (size_t)e->nmb * sizeof(MbInfo); break;
        case MI355X_H264_DBG_LEVELS: src = e->d_levels; n = (size_t)e->nmb * LV_STRIDE * 2; break;
        case MI355X_H264_DBG_MBAUX: src = e->d_aux; n = (size_t)e->nmb * 16; break;
        case MI355X_H264_DBG_MVQ: src = e->d_mvq; n = (size_t)e->nmb * 16; break;
        case MI355X_H264_DBG_SRC:   // the staging picture, where the kernels read the last picture from it
            if (e->last_src != e->d_stage)
                return set_err(e->err, MI355X_H264_E_ARG, "%s", e->last_src ? "the last picture was read in place from the caller's device memory: no staging picture" : "no picture yet");
            src = e->d_stage; n = e->frame_bytes; break;
        default: return MI355X_H264_E_ARG;
    }
    if (cap < n) return MI355X_H264_E_ARG;
    if (hipStreamSynchronize(e->stream) != hipSuccess) return MI355X_H264_E_HIP;
    if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return MI355X_H264_E_HIP;
    return (int64_t)n;
}

int mi355x_h264_debug_code_syntax(mi355x_h264_encoder* e, const void* mbinfo, const void* levels, const void* mvq, const void* mbaux,
                                  const uint8_t* src_i420, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    NEED(e, mbinfo && levels && mvq && mbaux && src_i420 && out && out_len, "null argument");
    NEED(e, e->cfg.band_count <= 1, "not for slice bands over several instances");
    NEED(e, e->seq.layers == 1, "not for an encoder with two temporal layers");
    NEED(e, !e->shape.refresh, "not for an encoder with intra refresh");
    HIPCHK(e->err, hipSetDevice(e->device));
    const size_t src_bytes = e->frame_bytes * (size_t)e->G;
    if (!e->d_inject_src) HIPCHK(e->err, DM_DEV(e->mem, e->d_inject_src, src_bytes + 256, false));
    HIPCHK(e->err, hipMemcpy(e->d_inject_src, src_i420, src_bytes, hipMemcpyHostToDevice));   // k_cavlc reads the I_PCM samples from the source
    const int slot = take_slot(e);
    const Injected inj{mbinfo, levels, mvq, mbaux};
    quality_begin(e, (size_t)e->G, 1, 0);
    int rc = submit(e, e->d_inject_src, e->frame_bytes, slot, false, &inj);
    if (rc) return rc;
    rc = wait_slot(e, slot);
    if (rc) return rc;
    char first[sizeof(e->err)] = {0};
    for (int g = 0; g < e->G; g++) {   // every item is finished, whatever became of the ones before it
        out[g] = nullptr; out_len[g] = 0;
        const int r = finish_item(e, e->slots[slot], e->slots[slot].lay, e->slots[slot].pics[g], &out[g], &out_len[g], frame_type);
        if (r) { out[g] = nullptr; out_len[g] = 0; }
        if (r && !rc) { rc = r; memcpy(first, e->err, sizeof(first)); }
    }
    if (rc) memcpy(e->err, first, sizeof(first));
    return rc;
}

int mi355x_h264_stats_enable(mi355x_h264_encoder* e, int on) { if (!e) return MI355X_H264_E_ARG; e->stats_on = on != 0; return MI355X_H264_OK; }

int mi355x_h264_stats_read(mi355x_h264_encoder* e, mi355x_h264_stats* out, int reset)
{
    if (!e || !out) return MI355X_H264_E_ARG;
    *out = e->stats;
    if (reset) memset(&e->stats, 0, sizeof(e->stats));
    return MI355X_H264_OK;
}

// ---- quality report (engine.h: quality_record; k_quality.h) ----

int mi355x_h264_quality_enable(mi355x_h264_encoder* e, int on)
{
    if (!e) return MI355X_H264_E_ARG;
    return quality_set(e, on != 0 ? MI355X_H264_QUALITY_SSE : 0u);
}

int mi355x_h264_quality_enable_ex(mi355x_h264_encoder* e, unsigned metrics)
{
    if (!e) return MI355X_H264_E_ARG;
    return quality_set(e, metrics);
}

int64_t mi355x_h264_quality_ssim_read(mi355x_h264_encoder* e, mi355x_h264_ssim* dst, size_t cap)
{
    NEED(e, dst, "null argument");
    NEED(e, !e->s_recs.empty(), "no quality SSIM records: SSIM was not enabled for the last call, or there has been no picture yet");
    NEED(e, cap >= e->s_recs.size(), "room for fewer records than the last call made");
    memcpy(dst, e->s_recs.data(), e->s_recs.size() * sizeof(mi355x_h264_ssim));
    return (int64_t)e->s_recs.size();
}

int64_t mi355x_h264_quality_ssim_map(mi355x_h264_encoder* e, int item, int32_t* dst, size_t cap)
{
    NEED(e, dst && item >= 0 && item < e->G, "null argument or no such item");
    NEED(e, !e->s_recs.empty() && e->s_have[item] && e->s_map[item], "no quality SSIM map: nothing was compared for the item's last picture");
    NEED(e, cap >= (size_t)e->nmb, "room for fewer entries than the picture has macroblocks");
    memcpy(dst, e->s_map[item], (size_t)e->nmb * sizeof(int32_t));
    return (int64_t)e->nmb;
}

int64_t mi355x_h264_quality_read(mi355x_h264_encoder* e, mi355x_h264_quality* dst, size_t cap)
{
    NEED(e, dst, "null argument");
    NEED(e, !e->q_recs.empty(), "no quality records: the report was not enabled for the last call, or there has been no picture yet");
    NEED(e, cap >= e->q_recs.size(), "room for fewer records than the last call made");
    memcpy(dst, e->q_recs.data(), e->q_recs.size() * sizeof(mi355x_h264_quality));
    return (int64_t)e->q_recs.size();
}

int64_t mi355x_h264_quality_map(mi355x_h264_encoder* e, int item, uint32_t* dst, size_t cap)
{
    NEED(e, dst && item >= 0 && item < e->G, "null argument or no such item");
    NEED(e, !e->q_recs.empty() && e->q_have[item] && e->q_map[item], "no quality map: nothing was compared for the item's last picture");
    NEED(e, cap >= (size_t)e->nmb, "room for fewer entries than the picture has macroblocks");
    memcpy(dst, e->q_map[item], (size_t)e->nmb * sizeof(uint32_t));
    return (int64_t)e->nmb;
}

// ---- streams (hub.h) ----

int mi355x_h264_stream_open(const mi355x_h264_config* cfg, mi355x_h264_stream** out) { return mi355x_h264_stream_open_ex(cfg, 0, out); }

int mi355x_h264_stream_open_ex(const mi355x_h264_config* cfg, uint32_t flags, mi355x_h264_stream** out)
{
    if (!cfg || !out || cfg->struct_size != sizeof(mi355x_h264_config)) return MI355X_H264_E_ARG;
    return mi355x_h264_stream_open_scaled(cfg, flags, cfg->width, cfg->height, out);
}

int mi355x_h264_stream_open_scaled(const mi355x_h264_config* cfg, uint32_t flags, int sw, int sh, mi355x_h264_stream** out)
{
    return mi355x_h264_stream_open_colour(cfg, flags, sw, sh, nullptr, out);
}

int mi355x_h264_stream_colour(const mi355x_h264_stream* s, mi355x_h264_colour* out) { return s && out ? colour_give(s->hub->colour, out) : MI355X_H264_E_ARG; }

int mi355x_h264_stream_open_colour(const mi355x_h264_config* cfg, uint32_t flags, int sw, int sh, const mi355x_h264_colour* colour, mi355x_h264_stream** out)
{
    if (!cfg || !out || cfg->struct_size != sizeof(mi355x_h264_config)) return MI355X_H264_E_ARG;
    *out = nullptr;
    ColourDesc desc;
    if (!colour_take(colour, &desc)) return MI355X_H264_E_ARG;
    if (sw != cfg->width || sh != cfg->height) {   // (the same size: exactly mi355x_h264_stream_open_ex, whatever it makes of the size)
        if (((sw | sh) & 1) || sw < 16 || sh < 16 || sw > 4096 || sh > 4096) return MI355X_H264_E_ARG;
        if (cfg->width < 16 || cfg->height < 16 || ((cfg->width | cfg->height) & 1)) return MI355X_H264_E_ARG;
        if (sw < cfg->width || sh < cfg->height || sw > 4 * cfg->width || sh > 4 * cfg->height) return MI355X_H264_E_ARG;
    }
    if (flags & ~(uint32_t)(MI355X_H264_STREAM_MULTIREF | MI355X_H264_STREAM_TEMPORAL2 | MI355X_H264_STREAM_INTRA_REFRESH)) return MI355X_H264_E_ARG;
    const bool refresh = (flags & MI355X_H264_STREAM_INTRA_REFRESH) != 0;
    // intra refresh: 2..32 bands of two rows or more that the picture really divides into, one reference picture, one layer
    if (refresh && ((flags & MI355X_H264_STREAM_TEMPORAL2) || cfg->refs > 1 || cfg->slices < 2 || refresh_bands((cfg->height + 15) / 16, cfg->slices) != cfg->slices))
        return MI355X_H264_E_ARG;
    const int max_refs = (flags & MI355X_H264_STREAM_MULTIREF) ? (int)mi355x_h264_encoder::MAX_REFS : 1;
    if (cfg->refs > max_refs || cfg->band_count > 1 || cfg->batch > 1) return MI355X_H264_E_ARG;
    if (cfg->input_format != MI355X_H264_INPUT_I420 && cfg->input_format != MI355X_H264_INPUT_NV12 && cfg->input_format != MI355X_H264_INPUT_RGBA)
        return MI355X_H264_E_ARG;
    if (cfg->qp < 10 || cfg->qp > 51 || cfg->gop < 1) return MI355X_H264_E_ARG;
    mi355x_h264_stream* s = new (std::nothrow) mi355x_h264_stream();
    if (!s) return MI355X_H264_E_NOMEM;
    std::lock_guard<std::mutex> gl(g_hubs_mu);
    Hub* h = nullptr;
    for (Hub* c : g_hubs)
        if (same_geometry(*c, *cfg, sw, sh, desc, refresh) && c->sched.has_room()) { h = c; break; }
    if (!h) {
        const int rc = hub_create(*cfg, sw, sh, desc, refresh, &h);
        if (rc != MI355X_H264_OK) { delete s; return rc; }
        g_hubs.push_back(h);
    }
    const int idx = h->sched.open(cfg->qp, cfg->gop, (flags & MI355X_H264_STREAM_TEMPORAL2) ? 2 : 1, refresh ? cfg->slices : 0);   // (there is room: opens and closes are serialised by g_hubs_mu)
    HubItem& it = h->items[idx];
    hipEvent_t ev = it.copied;
    it = HubItem();
    it.copied = ev;
    g_streams_open.fetch_add(1);
    if (!h->e->q_have.empty()) h->e->q_have[idx] = 0;   // (quality report: the item's record was the stream's before this one)
    if (!h->e->s_have.empty()) h->e->s_have[idx] = 0;
    s->hub = h; s->item = idx;
    *out = s;
    return MI355X_H264_OK;
}

void mi355x_h264_stream_close(mi355x_h264_stream* s)
{
    if (!s) return;
    std::lock_guard<std::mutex> gl(g_hubs_mu);
    Hub* h = s->hub;
    g_streams_open.fetch_sub(1);
    if (h->sched.close(s->item)) {   // the last one: no step is in flight any more
        g_hubs.erase(std::find(g_hubs.begin(), g_hubs.end(), h));
        hub_free(h);
    }
    delete s;
}

int mi355x_h264_stream_encode(mi355x_h264_stream* s, const uint8_t* y, int ys, const uint8_t* u, int us, const uint8_t* v, int vs,
                              uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !y || !u || !v || !out || !out_len) return MI355X_H264_E_ARG;
    return hub_encode(s, HostPicture{PIC_I420, {y, u, v}, {ys, us, vs}}, out, out_len, frame_type);
}

int mi355x_h264_stream_encode_nv12(mi355x_h264_stream* s, const uint8_t* y, int ys, const uint8_t* uv, int uvs, uint8_t** out, uint32_t* out_len,
                                   int* frame_type)
{
    if (!s || !y || !uv || !out || !out_len) return MI355X_H264_E_ARG;
    return hub_encode(s, HostPicture{PIC_NV12, {y, uv, nullptr}, {ys, uvs, 0}}, out, out_len, frame_type);
}

int mi355x_h264_stream_encode_rgba(mi355x_h264_stream* s, const uint8_t* rgba, int stride, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !rgba || !out || !out_len) return MI355X_H264_E_ARG;
    return hub_encode(s, HostPicture{PIC_RGBA, {rgba, nullptr, nullptr}, {stride, 0, 0}}, out, out_len, frame_type);
}

// damage tiles (hub.h, damage.h): the host calls with a damage set; every refusal leaves the stream as it was
int mi355x_h264_stream_encode_damage(mi355x_h264_stream* s, const uint8_t* y, int ys, const uint8_t* u, int us, const uint8_t* v, int vs,
                                     const mi355x_h264_rect* rects, int n, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !y || !u || !v || !out || !out_len) return MI355X_H264_E_ARG;
    const DamageReq d{rects, n};
    return hub_encode(s, HostPicture{PIC_I420, {y, u, v}, {ys, us, vs}}, out, out_len, frame_type, &d);
}

int mi355x_h264_stream_encode_nv12_damage(mi355x_h264_stream* s, const uint8_t* y, int ys, const uint8_t* uv, int uvs, const mi355x_h264_rect* rects, int n,
                                          uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !y || !uv || !out || !out_len) return MI355X_H264_E_ARG;
    const DamageReq d{rects, n};
    return hub_encode(s, HostPicture{PIC_NV12, {y, uv, nullptr}, {ys, uvs, 0}}, out, out_len, frame_type, &d);
}

int mi355x_h264_stream_encode_rgba_damage(mi355x_h264_stream* s, const uint8_t* rgba, int stride, const mi355x_h264_rect* rects, int n,
                                          uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !rgba || !out || !out_len) return MI355X_H264_E_ARG;
    const DamageReq d{rects, n};
    return hub_encode(s, HostPicture{PIC_RGBA, {rgba, nullptr, nullptr}, {stride, 0, 0}}, out, out_len, frame_type, &d);
}

// (the stream's calls are synchronous and only they write the item's record: read without the hub's lock, as last_error is)
int mi355x_h264_stream_last_upload(const mi355x_h264_stream* s, uint64_t* bytes, uint32_t* tiles, uint32_t* tiles_total, int* mode)
{
    if (!s) return MI355X_H264_E_ARG;
    const HubItem& it = s->hub->items[s->item];
    if (bytes) *bytes = it.up_bytes;
    if (tiles) *tiles = it.up_tiles;
    if (tiles_total) *tiles_total = (uint32_t)damage::tiles_total(s->hub->sw, s->hub->sh);
    if (mode) *mode = it.up_mode;
    return MI355X_H264_OK;
}

int mi355x_h264_stream_debug_patch_stats(const mi355x_h264_stream* s, uint64_t* launches, uint64_t* tiles)
{
    if (!s) return MI355X_H264_E_ARG;
    if (launches) *launches = s->hub->patch_launches.load();
    if (tiles) *tiles = s->hub->patch_tiles.load();
    return MI355X_H264_OK;
}

int mi355x_h264_stream_encode_device(mi355x_h264_stream* s, const void* d_pic, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    if (!s || !d_pic || !out || !out_len) return MI355X_H264_E_ARG;
    return hub_encode(s, HostPicture{HUB_IN_DEVICE, {(const uint8_t*)d_pic, nullptr, nullptr}, {0, 0, 0}}, out, out_len, frame_type);
}

int mi355x_h264_stream_set_qp(mi355x_h264_stream* s, int qp) { if (!s || qp < 10 || qp > 51) return MI355X_H264_E_ARG; s->hub->sched.set_qp(s->item, qp); return MI355X_H264_OK; }
int mi355x_h264_stream_force_idr(mi355x_h264_stream* s) { if (!s) return MI355X_H264_E_ARG; s->hub->sched.force_idr(s->item); return MI355X_H264_OK; }
int mi355x_h264_stream_set_idr_pic_id(mi355x_h264_stream* s, int next) { if (!s) return MI355X_H264_E_ARG; s->hub->sched.set_idr_pic_id(s->item, next); return MI355X_H264_OK; }

int mi355x_h264_stream_last_me_cost(const mi355x_h264_stream* s, uint32_t* cost) { if (!s || !cost) return MI355X_H264_E_ARG; *cost = s->hub->e->last_me_cost[s->item]; return MI355X_H264_OK; }

const char* mi355x_h264_stream_last_error(const mi355x_h264_stream* s) { return s ? s->hub->items[s->item].err : "null stream"; }
int mi355x_h264_stream_coded_width(const mi355x_h264_stream* s) { return s ? s->hub->e->cw : 0; }
int mi355x_h264_stream_coded_height(const mi355x_h264_stream* s) { return s ? s->hub->e->ch : 0; }
int mi355x_h264_stream_source_width(const mi355x_h264_stream* s) { return s ? s->hub->sw : 0; }
int mi355x_h264_stream_source_height(const mi355x_h264_stream* s) { return s ? s->hub->sh : 0; }

// test hooks: what mi355x_h264_debug_read gives for an engine, for the stream's own batch item after its last picture; the stream's
// calls are synchronous, so the picture is complete, and nothing rewrites the item's arrays before the stream's next call
int64_t mi355x_h264_stream_debug_read(mi355x_h264_stream* s, int what, void* dst, size_t cap)
{
    if (!s || !dst) return MI355X_H264_E_ARG;
    Hub* h = s->hub;
    const mi355x_h264_encoder* e = h->e;
    if (hipSetDevice(h->cfg.device) != hipSuccess) return MI355X_H264_E_HIP;
    const size_t ysz = (size_t)e->cw * e->ch, item = (size_t)s->item, mb0 = item * e->nmb;
    const void* src = nullptr;
    size_t n = 0;
    switch (what) {
        case MI355X_H264_DBG_RECON_Y: case MI355X_H264_DBG_RECON_U: case MI355X_H264_DBG_RECON_V:
            src = e->d_plane_base[what] + item * (what ? e->st_c : e->st_y) + (size_t)h->sched.last_cur(s->item) * (what ? e->st_ring_c : e->st_ring_y);
            n = what ? ysz / 4 : ysz; break;
        case MI355X_H264_DBG_PRE_Y: case MI355X_H264_DBG_PRE_U: case MI355X_H264_DBG_PRE_V: {
            const int p = what - MI355X_H264_DBG_PRE_Y;
            src = e->d_pre[p] + item * (p ? e->st_ring_c : e->st_ring_y); n = p ? ysz / 4 : ysz; break;
        }
        case MI355X_H264_DBG_MBINFO: src = e->d_mb + mb0; n = (size_t)e->nmb * sizeof(MbInfo); break;
        case MI355X_H264_DBG_LEVELS: src = e->d_levels + mb0 * LV_STRIDE; n = (size_t)e->nmb * LV_STRIDE * 2; break;
        case MI355X_H264_DBG_MBAUX: src = e->d_aux + mb0 * 16; n = (size_t)e->nmb * 16; break;
        case MI355X_H264_DBG_MVQ: src = e->d_mvq + mb0 * 8; n = (size_t)e->nmb * 16; break;
        case MI355X_H264_DBG_SRC: {   // the stream's slot of the hub's staging pictures, where the step's kernels read the last picture from it
            HubItem& it = h->items[s->item];
            uint64_t serial = 0;
            h->sched.last_step(s->item, &serial, nullptr, nullptr, nullptr);
            if (!serial || it.d_in)
                return set_err(it.err, MI355X_H264_E_ARG, "%s", serial ? "the last picture was read in place from the caller's device memory: no staging picture" : "no picture yet");
            src = h->d_stage + item * h->st_stage; n = e->frame_bytes; break;
        }
        default: return MI355X_H264_E_ARG;
    }
    if (cap < n) return MI355X_H264_E_ARG;
    if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return MI355X_H264_E_HIP;
    return (int64_t)n;
}

// keeps a copy of every picture's reconstruction before the loop filter, for all streams of this stream's engine (engine.h, submit_step)
int mi355x_h264_stream_debug_keep_pre(mi355x_h264_stream* s, int on)
{
    if (!s) return MI355X_H264_E_ARG;
    std::lock_guard<std::mutex> lk(s->hub->launch_mu);   // (a step's leader reads it while it launches)
    s->hub->e->keep_pre = on != 0;
    return MI355X_H264_OK;
}

// the quality report of all streams of this stream's engine (engine.h, submit_step), and this stream's last record and map
int mi355x_h264_stream_quality_enable_ex(mi355x_h264_stream* s, unsigned metrics)
{
    if (!s) return MI355X_H264_E_ARG;
    if (hipSetDevice(s->hub->cfg.device) != hipSuccess) return set_err(s->hub->items[s->item].err, MI355X_H264_E_HIP, "hipSetDevice");
    std::lock_guard<std::mutex> lk(s->hub->launch_mu);   // (a step's leader reads the switch while it launches, and the records when it finishes)
    const int rc = quality_set(s->hub->e, metrics);
    if (rc != MI355X_H264_OK) snprintf(s->hub->items[s->item].err, sizeof(s->hub->items[s->item].err), "%s", s->hub->e->err);
    return rc;
}
int mi355x_h264_stream_quality_enable(mi355x_h264_stream* s, int on) { return mi355x_h264_stream_quality_enable_ex(s, on != 0 ? MI355X_H264_QUALITY_SSE : 0u); }

int mi355x_h264_stream_last_ssim(const mi355x_h264_stream* s, mi355x_h264_ssim* out)
{
    if (!s) return MI355X_H264_E_ARG;
    Hub* h = s->hub;
    if (!out) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->launch_mu);
    if (h->e->s_have.empty() || !h->e->s_have[s->item])
        return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "no quality SSIM record: SSIM was not enabled for the stream's last picture, or there has been no picture yet");
    *out = h->e->s_item[s->item];
    return MI355X_H264_OK;
}

int64_t mi355x_h264_stream_ssim_map(mi355x_h264_stream* s, int32_t* dst, size_t cap)
{
    if (!s) return MI355X_H264_E_ARG;
    Hub* h = s->hub;
    const mi355x_h264_encoder* e = h->e;
    if (!dst) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->launch_mu);
    if (e->s_have.empty() || !e->s_have[s->item] || !e->s_map[s->item])
        return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "no quality SSIM map: nothing was compared for the stream's last picture");
    if (cap < (size_t)e->nmb) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "room for fewer entries than the picture has macroblocks");
    memcpy(dst, e->s_map[s->item], (size_t)e->nmb * sizeof(int32_t));   // (as mi355x_h264_stream_quality_map: nothing rewrites this before the stream's next picture)
    return (int64_t)e->nmb;
}

int mi355x_h264_stream_last_quality(const mi355x_h264_stream* s, mi355x_h264_quality* out)
{
    if (!s) return MI355X_H264_E_ARG;
    Hub* h = s->hub;
    if (!out) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->launch_mu);
    if (h->e->q_have.empty() || !h->e->q_have[s->item])
        return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "no quality record: the report was not enabled for the stream's last picture, or there has been no picture yet");
    *out = h->e->q_item[s->item];
    return MI355X_H264_OK;
}

int64_t mi355x_h264_stream_quality_map(mi355x_h264_stream* s, uint32_t* dst, size_t cap)
{
    if (!s) return MI355X_H264_E_ARG;
    Hub* h = s->hub;
    const mi355x_h264_encoder* e = h->e;
    if (!dst) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->launch_mu);
    if (e->q_have.empty() || !e->q_have[s->item] || !e->q_map[s->item])
        return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "no quality map: nothing was compared for the stream's last picture");
    if (cap < (size_t)e->nmb) return set_err(h->items[s->item].err, MI355X_H264_E_ARG, "room for fewer entries than the picture has macroblocks");
    // (the stream's calls are synchronous and a step stores only its own items' part of the pinned arrays: nothing rewrites this before the stream's next picture)
    memcpy(dst, e->q_map[s->item], (size_t)e->nmb * sizeof(uint32_t));
    return (int64_t)e->nmb;
}

int mi355x_h264_stream_debug_last_step(const mi355x_h264_stream* s, uint64_t* serial, int* pictures, int* position, int* idr)
{
    if (!s) return MI355X_H264_E_ARG;
    s->hub->sched.last_step(s->item, serial, pictures, position, idr);
    return MI355X_H264_OK;
}

// how the hub of this stream has been batching: steps launched, pictures coded, the largest step
int mi355x_h264_stream_hub_stats(const mi355x_h264_stream* s, uint64_t* steps, uint64_t* pictures, uint64_t* max_batch, int* open_streams)
{
    if (!s) return MI355X_H264_E_ARG;
    HubSched& h = s->hub->sched;
    std::lock_guard<std::mutex> lk(h.mu);
    if (steps) *steps = h.steps;
    if (pictures) *pictures = h.pictures;
    if (max_batch) *max_batch = h.max_batch;
    if (open_streams) *open_streams = h.nopen;
    return MI355X_H264_OK;
}

// ---- decoder groups (dec_group.h) ----

int mi355x_h264_dec_group_create(int device, int streams, mi355x_h264_dec_group** out)
{
    if (!out) return MI355X_H264_E_ARG;
    *out = nullptr;
    if (streams < 1 || streams > DEC_GROUP_MAX_STREAMS) return MI355X_H264_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return MI355X_H264_E_NODEVICE;
    mi355x_h264_dec_group* g = new (std::nothrow) mi355x_h264_dec_group();
    if (!g) return MI355X_H264_E_NOMEM;
    g->device = device; g->nstreams = streams;
    g->mem.configure(); g->store.mem.configure();   // the guard mode of dev_mem.h, as the process-wide switch stands now
    g->st = new (std::nothrow) DecGroupStream[streams];
    if (!g->st) { delete g; return MI355X_H264_E_NOMEM; }
    if (hipSetDevice(device) != hipSuccess || hipEventCreateWithFlags(&g->up_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g->up_done[1], hipEventDisableTiming) != hipSuccess || sync_create(g->sync, nullptr, nullptr, true) != hipSuccess) {
        for (hipEvent_t ev : g->up_done) if (ev) (void)hipEventDestroy(ev);
        sync_destroy(g->sync);
        delete[] g->st;
        delete g;
        return MI355X_H264_E_HIP;
    }
    // pictures the row wavefronts hold at a time; a step of more walks to the rest (k_pintra_rows, k_deblock_rows)
    g->intra_slots = env_int("MI355X_H264_DEC_INTRA_SLOTS", 1, DEC_GROUP_MAX_STREAMS, 32);
    g->filter_slots = env_int("MI355X_H264_DEC_FILTER_SLOTS", 1, DEC_GROUP_MAX_STREAMS, 32);
    // the parse threads: a number of the group's own, never the machine's; one stream is parsed by the caller (dec_group_sched.h)
    if (streams > 1) g->sched.start(env_int("MI355X_H264_DEC_PARSE_THREADS", 1, DEC_GROUP_MAX_THREADS, std::min(streams, 8)));
    *out = g;
    return MI355X_H264_OK;
}

void mi355x_h264_dec_group_destroy(mi355x_h264_dec_group* g)
{
    if (!g) return;
    g->sched.stop();
    (void)hipSetDevice(g->device);
    (void)dg_wait(g);
    (void)hipStreamSynchronize(g->sync.st);   // (an armed step's copy, the uploads out of both pinned sets)
    dg_free_geometry(g);
    for (int k = 0; k < 2; k++) {
        if (g->up_done[k]) (void)hipEventDestroy(g->up_done[k]);
        if (g->out.done[k]) (void)hipEventDestroy(g->out.done[k]);
    }
    sync_destroy(g->sync);
    delete[] g->st;
    delete g;
}

// No exception leaves the C entry point; a failure that concerns the whole group (device, allocation, a timed-out wavefront) may have
// cost any stream a reference picture, so all of them then wait for their next IDR picture.
int mi355x_h264_dec_group_decode(mi355x_h264_dec_group* g, const uint8_t* const* aus, const size_t* lens, int* got, int* rc)
{
    if (!g || !aus || !lens || !got || !rc) return MI355X_H264_E_ARG;
    int r;
    try {
        r = dg_step(g, aus, lens, got, rc);
    } catch (const std::exception& ex) {
        r = set_err(g->err, MI355X_H264_E_NOMEM, "step refused: %s", ex.what());
    }
    if (r != MI355X_H264_OK)
        for (int i = 0; i < g->nstreams; i++) {
            if (aus[i]) { got[i] = 0; if (rc[i] == MI355X_H264_OK) rc[i] = r; dg_drop_refs(g->st[i]); }
        }
    return r;
}

int mi355x_h264_dec_group_sync(mi355x_h264_dec_group* g)
{
    if (!g) return MI355X_H264_E_ARG;
    if (!g->store.made()) return MI355X_H264_OK;
    if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
    return dg_wait(g);
}

// stream -1: the group's own report (what made a call return < 0)
const char* mi355x_h264_dec_group_last_error(const mi355x_h264_dec_group* g, int stream)
{
    if (!g) return "no decoder group";
    if (stream == -1) return g->err;
    if (stream < 0 || stream >= g->nstreams) return "no such stream";
    return g->st[stream].err;
}

int mi355x_h264_dec_group_picture_info(const mi355x_h264_dec_group* g, int stream, int* w, int* h, int* cw, int* ch)
{
    if (!g || stream < 0 || stream >= g->nstreams || g->st[stream].last < 0) return MI355X_H264_E_ARG;
    if (w) *w = g->st[stream].width;
    if (h) *h = g->st[stream].height;
    if (cw) *cw = g->store.cw;
    if (ch) *ch = g->store.ch;
    return MI355X_H264_OK;
}

// out[8] of mi355x_h264_dec_colour from a sequence parameter set's VUI (an absent VUI: the absent values of h264dec::Vui)
static void vui_report(const h264dec::Vui& v, int32_t* out)
{
    out[0] = v.colour ? 1 : 0; out[1] = v.matrix; out[2] = v.full_range; out[3] = v.primaries; out[4] = v.transfer;
    out[5] = v.chroma_loc; out[6] = v.fps(); out[7] = v.reorder;
}

int mi355x_h264_dec_group_colour(const mi355x_h264_dec_group* g, int stream, int32_t* out)
{
    if (!g || !out || stream < 0 || stream >= g->nstreams || g->st[stream].last < 0) return MI355X_H264_E_ARG;
    vui_report(g->st[stream].vui, out);
    return MI355X_H264_OK;
}

int mi355x_h264_dec_group_set_rgba_colour(mi355x_h264_dec_group* g, int stream, const mi355x_h264_colour* colour)
{
    if (!g || stream < 0 || stream >= g->nstreams) return MI355X_H264_E_ARG;
    ColourDesc d;
    if (!colour_take(colour, &d)) return MI355X_H264_E_ARG;
    g->st[stream].rgba_override = d.described ? colour_variant(d.matrix, d.full_range) : -1;
    return MI355X_H264_OK;
}

int64_t mi355x_h264_dec_group_read_i420(mi355x_h264_dec_group* g, int stream, uint8_t* dst, size_t cap) { return dg_read(g, stream, dst, cap, false); }
int64_t mi355x_h264_dec_group_read_i420_device(mi355x_h264_dec_group* g, int stream, void* d_dst, size_t cap) { return dg_read(g, stream, d_dst, cap, true); }

int64_t mi355x_h264_dec_group_debug_plane(mi355x_h264_dec_group* g, int stream, int plane, void* dst, size_t cap)
{
    if (!g || !dst || stream < 0 || stream >= g->nstreams || g->st[stream].last < 0 || plane < 0 || plane > 2) return MI355X_H264_E_ARG;
    const PicStore* const ps = &g->store;
    const size_t n = (size_t)ps->cw * ps->ch / (plane ? 4 : 1);
    if (cap < n) return MI355X_H264_E_ARG;
    if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
    if (const int wrc = dg_wait(g)) return wrc;
    const uint8_t* src = ps->d_plane_base[plane] + (size_t)stream * (plane ? ps->st_c : ps->st_y) + (size_t)g->st[stream].last * (plane ? ps->st_ring_c : ps->st_ring_y);
    if (hipMemcpy(dst, src, n, hipMemcpyDeviceToHost) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipMemcpy");
    return (int64_t)n;
}

int mi355x_h264_dec_group_last_step(const mi355x_h264_dec_group* g, int64_t* out, int n)
{
    if (!g || !out || n < 1) return MI355X_H264_E_ARG;
    const int m = n >= 13 ? 13 : (n >= 11 ? 11 : (n >= 9 ? 9 : std::min(n, 7)));   // (a caller with an earlier layout's slots gets those)
    for (int i = 0; i < std::min(m, 11); i++) out[i] = g->last[i];
    if (m == 13) {   // what the group holds now: the store's and its own (the parsers' heap is not counted)
        out[11] = (int64_t)(g->store.mem.dev_bytes + g->mem.dev_bytes);
        out[12] = (int64_t)(g->store.mem.pinned_bytes + g->mem.pinned_bytes);
    }
    return m;
}

int64_t mi355x_h264_dec_group_read_all(mi355x_h264_dec_group* g, int layout, int row_align, void* dst, size_t cap, int to_device, mi355x_h264_dec_out_pic* pics)
{
    return dg_read_all(g, layout, row_align, dst, cap, to_device != 0, pics);
}
int mi355x_h264_dec_group_set_output(mi355x_h264_dec_group* g, int layout, int row_align) { return dg_set_output(g, layout, row_align); }
int mi355x_h264_dec_group_output(mi355x_h264_dec_group* g, int back, const uint8_t** data, mi355x_h264_dec_out_pic* pics) { return dg_output(g, back, data, pics); }

// the size a stream's pictures are delivered at (k_dec_out_scale.h); nothing on the device is touched: the next call's table says it
int mi355x_h264_dec_group_set_output_size(mi355x_h264_dec_group* g, int stream, int width, int height)
{
    if (!g || stream < -1 || stream >= g->nstreams || !out_size_ok(width, height)) return MI355X_H264_E_ARG;
    for (int i = 0; i < g->nstreams; i++)
        if (stream == -1 || stream == i) { g->st[i].out_w = width; g->st[i].out_h = height; }
    return MI355X_H264_OK;
}
int mi355x_h264_dec_group_output_size(const mi355x_h264_dec_group* g, int stream, int* width, int* height)
{
    if (!g || !width || !height || stream < 0 || stream >= g->nstreams) return MI355X_H264_E_ARG;
    *width = g->st[stream].out_w; *height = g->st[stream].out_h;
    return MI355X_H264_OK;
}

// ---- loss mode (dec_group.h, dec_loss.h): the switch, and what the host knows about the damage in a stream's last picture ----
int mi355x_h264_dec_group_set_loss_mode(mi355x_h264_dec_group* g, int stream, int mode)
{
    if (!g || stream < 0 || stream >= g->nstreams || mode < MI355X_H264_LOSS_STRICT || mode > MI355X_H264_LOSS_CONCEAL) return MI355X_H264_E_ARG;
    DecGroupStream& s = g->st[stream];
    s.loss = mode;
    s.parser.set_conceal(mode == MI355X_H264_LOSS_CONCEAL);
    return MI355X_H264_OK;
}
int mi355x_h264_dec_group_damage(const mi355x_h264_dec_group* g, int stream, int32_t* out)
{
    if (!g || !out || stream < 0 || stream >= g->nstreams) return MI355X_H264_E_ARG;
    const DecGroupStream& s = g->st[stream];
    const bool c = s.loss != 0 || !s.taint.empty();   // (a stream that has concealed keeps its maps, whatever its mode is now)
    out[0] = c ? s.tainted : 0; out[1] = c ? s.concealed : 0; out[2] = c ? s.gap : 0; out[3] = s.last < 0 ? -1 : s.recovery;
    out[4] = (int32_t)std::min<int64_t>(s.since, 0x7FFFFFFF); out[5] = c && s.joined ? 1 : 0;
    return MI355X_H264_OK;
}
int64_t mi355x_h264_dec_group_damage_map(const mi355x_h264_dec_group* g, int stream, uint8_t* dst, size_t cap)
{
    if (!g || !dst || stream < 0 || stream >= g->nstreams || g->st[stream].last < 0) return MI355X_H264_E_ARG;
    const DecGroupStream& s = g->st[stream];
    const size_t nmb = (size_t)g->store.nmb;
    if (cap < nmb) return MI355X_H264_E_ARG;
    if (s.taint.size() == nmb * (size_t)g->store.nbuf) memcpy(dst, s.taint.data() + (size_t)s.last * nmb, nmb);
    else memset(dst, 0, nmb);
    return (int64_t)nmb;
}

// ---- the decoder peer (decoder.h): a group of one stream, every call forwarded with stream 0 ----

int mi355x_h264_dec_create(int device, mi355x_h264_decoder** out)
{
    if (!out) return MI355X_H264_E_ARG;
    *out = nullptr;
    mi355x_h264_decoder* d = new (std::nothrow) mi355x_h264_decoder();
    if (!d) return MI355X_H264_E_NOMEM;
    const int rc = mi355x_h264_dec_group_create(device, 1, &d->g);
    if (rc != MI355X_H264_OK) { delete d; return rc; }
    d->g->resize = true;   // an IDR picture of another coded size re-makes the geometry
    *out = d;
    return MI355X_H264_OK;
}

void mi355x_h264_dec_destroy(mi355x_h264_decoder* d)
{
    if (!d) return;
    mi355x_h264_dec_group_destroy(d->g);
    delete d;
}

const char* mi355x_h264_dec_last_error(const mi355x_h264_decoder* d) { return d ? d->err : "no decoder"; }

// An access unit that is refused at ANY stage - parser, stream checks, allocation, launch, the time-out of the picture in flight -
// may have been a reference picture: the group drops the parser's and the ring's reference pictures together (dg_drop_refs), so
// that every P picture is refused until the next IDR picture instead of being predicted from the wrong slot.
int mi355x_h264_dec_decode(mi355x_h264_decoder* d, const uint8_t* au, size_t len, int* got_picture)
{
    if (!d || !au) return MI355X_H264_E_ARG;
    mi355x_h264_dec_group* g = d->g;
    int got = 0, rc = MI355X_H264_OK;
    const int64_t before = g->step_serial;
    const int grc = mi355x_h264_dec_group_decode(g, &au, &len, &got, &rc);
    if (g->step_serial != before) { d->parse_ms += g->last_ms[0]; d->gpu_ms += g->last_ms[1]; }
    snprintf(d->err, sizeof(d->err), "%s", grc ? g->err : g->st[0].err);
    if (got_picture) *got_picture = got;
    return grc ? grc : rc;
}

int mi355x_h264_dec_sync(mi355x_h264_decoder* d) { return d ? dec_ret(d, mi355x_h264_dec_group_sync(d->g)) : MI355X_H264_E_ARG; }

int mi355x_h264_dec_picture_info(const mi355x_h264_decoder* d, int* width, int* height, int* coded_width, int* coded_height)
{
    return d ? mi355x_h264_dec_group_picture_info(d->g, 0, width, height, coded_width, coded_height) : MI355X_H264_E_ARG;
}

int mi355x_h264_dec_colour(const mi355x_h264_decoder* d, int32_t* out) { return d ? mi355x_h264_dec_group_colour(d->g, 0, out) : MI355X_H264_E_ARG; }
int mi355x_h264_dec_set_rgba_colour(mi355x_h264_decoder* d, const mi355x_h264_colour* colour) { return d ? mi355x_h264_dec_group_set_rgba_colour(d->g, 0, colour) : MI355X_H264_E_ARG; }

int64_t mi355x_h264_dec_read_i420(mi355x_h264_decoder* d, uint8_t* dst, size_t cap) { return d ? dec_ret(d, dg_read(d->g, 0, dst, cap, false)) : MI355X_H264_E_ARG; }
int64_t mi355x_h264_dec_read_i420_device(mi355x_h264_decoder* d, void* d_dst, size_t cap) { return d ? dec_ret(d, dg_read(d->g, 0, d_dst, cap, true)) : MI355X_H264_E_ARG; }

// the last picture in a layout: the group's call with one stream; `serial` counts the decoder's pictures, and the picture is
// always the one the last successful decode call produced
int64_t mi355x_h264_dec_read(mi355x_h264_decoder* d, int layout, int row_align, void* dst, size_t cap, int to_device, mi355x_h264_dec_out_pic* pic)
{
    if (!d) return MI355X_H264_E_ARG;
    const int64_t n = dec_ret(d, dg_read_all(d->g, layout, row_align, dst, cap, to_device != 0, pic));
    if (n >= 0) { pic->fresh = 1; pic->serial = (int64_t)d->g->st[0].pictures; }
    // (refused for the output size: the stream's report names both sizes)
    int W, H;
    if (n == MI355X_H264_E_ARG && pic && out_args_ok(layout, row_align) && d->g->st[0].last >= 0 && !dg_out_size(d->g->st[0], W, H)) snprintf(d->err, sizeof(d->err), "%s", d->g->st[0].err);
    return n;
}

int mi355x_h264_dec_set_loss_mode(mi355x_h264_decoder* d, int mode) { return d ? mi355x_h264_dec_group_set_loss_mode(d->g, 0, mode) : MI355X_H264_E_ARG; }
int mi355x_h264_dec_damage(const mi355x_h264_decoder* d, int32_t* out) { return d ? mi355x_h264_dec_group_damage(d->g, 0, out) : MI355X_H264_E_ARG; }
int64_t mi355x_h264_dec_damage_map(const mi355x_h264_decoder* d, uint8_t* dst, size_t cap) { return d ? mi355x_h264_dec_group_damage_map(d->g, 0, dst, cap) : MI355X_H264_E_ARG; }

int mi355x_h264_dec_set_output_size(mi355x_h264_decoder* d, int width, int height) { return d ? mi355x_h264_dec_group_set_output_size(d->g, 0, width, height) : MI355X_H264_E_ARG; }
int mi355x_h264_dec_output_size(const mi355x_h264_decoder* d, int* width, int* height) { return d ? mi355x_h264_dec_group_output_size(d->g, 0, width, height) : MI355X_H264_E_ARG; }

// coded-size planes of the last picture (test hook: compared with the oracle decoder's planes)
int64_t mi355x_h264_dec_debug_plane(mi355x_h264_decoder* d, int plane, void* dst, size_t cap)
{
    return d ? dec_ret(d, mi355x_h264_dec_group_debug_plane(d->g, 0, plane, dst, cap)) : MI355X_H264_E_ARG;
}

int mi355x_h264_dec_last_step(const mi355x_h264_decoder* d, int64_t* out, int n) { return d ? mi355x_h264_dec_group_last_step(d->g, out, n) : MI355X_H264_E_ARG; }

int mi355x_h264_dec_timing(const mi355x_h264_decoder* d, uint64_t* pictures, double* parse_ms, double* gpu_ms)
{
    if (!d) return MI355X_H264_E_ARG;
    if (pictures) *pictures = d->g->st[0].pictures;
    if (parse_ms) *parse_ms = d->parse_ms;
    if (gpu_ms) *gpu_ms = d->gpu_ms;
    return MI355X_H264_OK;
}

// ---- the guard mode of dev_mem.h: the process-wide switch, the tally of the free paths, a check and a poke per kind of owner ----
namespace {

// the lines of the report into the caller's buffer (cut where it ends, always terminated)
void mem_report(const std::vector<MemDamage>& found, size_t blocks, int slack, char* report, size_t cap)
{
    if (!report || !cap) return;
    report[0] = 0;
    const int h = snprintf(report, cap, "examined blocks=%zu slack=%d\n", blocks, slack);
    if (h < 0 || (size_t)h >= cap) { report[0] = 0; return; }
    size_t at = (size_t)h;
    for (const MemDamage& d : found) {
        const int n = snprintf(report + at, cap - at, "%s\n", d.line().c_str());
        if (n < 0 || (size_t)n >= cap - at) break;
        at += (size_t)n;
    }
}
// the check of an owner's lists (store: its ring slack as well); the owner's work has been waited for
int mem_check_lists(std::initializer_list<const DevMem*> lists, std::initializer_list<const PicStore*> stores, int* regions, char* report, size_t cap)
{
    std::vector<MemDamage> found;
    int looked = 0, slack = 0;
    size_t blocks = 0;
    for (const DevMem* m : lists) { if (m->check(found, &looked) < 0) return MI355X_H264_E_HIP; blocks += m->blocks.size(); }
    for (const PicStore* s : stores) if (store_check_slack(*s, found, &slack) < 0) return MI355X_H264_E_HIP;
    if (regions) *regions = looked + slack;
    mem_report(found, blocks, slack, report, cap);   // (what a check finds is the caller's to assert: the log is the free paths')
    return (int)found.size();
}
// block: a name (the first block of that name in the lists, in their order) or "#N" (block N of the lists laid end to end, from
// the back when N is negative: "#0" the first, "#-1" the last)
int mem_poke_lists(std::initializer_list<const DevMem*> lists, const char* block, int64_t offset, int value)
{
    if (!block) return MI355X_H264_E_ARG;
    std::vector<std::pair<const DevMem*, const DevMem::Block*>> all;
    for (const DevMem* m : lists) for (const DevMem::Block& b : m->blocks) all.push_back({m, &b});
    const std::pair<const DevMem*, const DevMem::Block*>* hit = nullptr;
    if (block[0] == '#') {
        long n = atol(block + 1);
        if (n < 0) n += (long)all.size();
        if (n >= 0 && n < (long)all.size()) hit = &all[(size_t)n];
    } else {
        for (const auto& a : all) if (!strcmp(a.second->name, block)) { hit = &a; break; }
    }
    if (!hit) return MI355X_H264_E_ARG;
    return hit->first->poke(*hit->second, offset, value) ? MI355X_H264_OK : MI355X_H264_E_ARG;
}

}  // namespace

int mi355x_h264_debug_mem_guard(int64_t guard_bytes, int poison)
{
    return mem_guard_set(guard_bytes, poison != 0) ? MI355X_H264_OK : MI355X_H264_E_ARG;
}

int mi355x_h264_debug_mem_guard_get(int64_t* guard_bytes, int* poison)
{
    const MemGuardSetting s = mem_guard_setting();
    if (guard_bytes) *guard_bytes = (int64_t)s.guard;
    if (poison) *poison = s.poison;
    return MI355X_H264_OK;
}

int64_t mi355x_h264_debug_mem_tally(int reset)
{
    std::atomic<unsigned long long>& t = mem_guard_global().tally;
    return (int64_t)(reset ? t.exchange(0) : t.load());
}

int mi355x_h264_debug_mem_check(mi355x_h264_encoder* e, int* regions, char* report, size_t cap)
{
    if (!e) return MI355X_H264_E_ARG;
    if (regions) *regions = 0;
    if (report && cap) report[0] = 0;
    NEED(e, e->mem.guard, "the encoder was created without guards (mi355x_h264_debug_mem_guard)");
    HIPCHK(e->err, hipSetDevice(e->device));
    HIPCHK(e->err, hipStreamSynchronize(e->stream));
    if (e->stream_ec != e->stream) HIPCHK(e->err, hipStreamSynchronize(e->stream_ec));
    const int n = mem_check_lists({&e->mem}, {e}, regions, report, cap);
    return n < 0 ? set_err(e->err, n, "guard check: a copy failed") : n;
}

int mi355x_h264_debug_mem_poke(mi355x_h264_encoder* e, const char* block, int64_t offset, int value)
{
    if (!e) return MI355X_H264_E_ARG;
    NEED(e, e->mem.guard, "the encoder was created without guards (mi355x_h264_debug_mem_guard)");
    HIPCHK(e->err, hipSetDevice(e->device));
    const int rc = mem_poke_lists({&e->mem}, block, offset, value);
    return rc ? set_err(e->err, rc, "no such block, or the offset is outside its guard regions") : rc;
}

// the hub's own blocks and the shared engine's; the steps of every stream of the hub are waited for (no stream of it may be in a
// call of its own meanwhile: the check is a test hook)
int mi355x_h264_stream_debug_mem_check(mi355x_h264_stream* s, int* regions, char* report, size_t cap)
{
    if (!s) return MI355X_H264_E_ARG;
    if (regions) *regions = 0;
    if (report && cap) report[0] = 0;
    Hub* h = s->hub;
    char (&err)[256] = h->items[s->item].err;
    if (!h->mem.guard || !h->e->mem.guard) return set_err(err, MI355X_H264_E_ARG, "the stream's hub was created without guards (mi355x_h264_debug_mem_guard)");
    std::lock_guard<std::mutex> lk(h->launch_mu);
    HIPCHK(err, hipSetDevice(h->cfg.device));
    HIPCHK(err, hipDeviceSynchronize());
    const int n = mem_check_lists({&h->mem, &h->e->mem}, {h->e}, regions, report, cap);
    return n < 0 ? set_err(err, n, "guard check: a copy failed") : n;
}

int mi355x_h264_dec_group_debug_mem_check(mi355x_h264_dec_group* g, int* regions, char* report, size_t cap)
{
    if (!g) return MI355X_H264_E_ARG;
    if (regions) *regions = 0;
    if (report && cap) report[0] = 0;
    if (!g->mem.guard) return set_err(g->err, MI355X_H264_E_ARG, "the group was created without guards (mi355x_h264_debug_mem_guard)");
    HIPCHK(g->err, hipSetDevice(g->device));
    if (const int wrc = dg_wait(g)) return wrc;
    HIPCHK(g->err, hipStreamSynchronize(g->sync.st));   // (an armed step's copy)
    const int n = mem_check_lists({&g->store.mem, &g->mem}, {&g->store}, regions, report, cap);
    return n < 0 ? set_err(g->err, n, "guard check: a copy failed") : n;
}

int mi355x_h264_dec_group_debug_mem_poke(mi355x_h264_dec_group* g, const char* block, int64_t offset, int value)
{
    if (!g) return MI355X_H264_E_ARG;
    if (!g->mem.guard) return set_err(g->err, MI355X_H264_E_ARG, "the group was created without guards (mi355x_h264_debug_mem_guard)");
    HIPCHK(g->err, hipSetDevice(g->device));
    const int rc = mem_poke_lists({&g->store.mem, &g->mem}, block, offset, value);
    return rc ? set_err(g->err, rc, "no such block, or the offset is outside its guard regions") : rc;
}

int mi355x_h264_dec_debug_mem_check(mi355x_h264_decoder* d, int* regions, char* report, size_t cap)
{
    if (!d) return MI355X_H264_E_ARG;
    const int rc = mi355x_h264_dec_group_debug_mem_check(d->g, regions, report, cap);
    if (rc < 0) snprintf(d->err, sizeof(d->err), "%s", d->g->err);   // (E_ARG too: "created without guards" is the group's text)
    return rc;
}

// ---- the host parser alone (no GPU): what it recovered from the last access unit, for the CPU tests ----
struct mi355x_h264_parser { h264dec::Parser p; };
mi355x_h264_parser* mi355x_h264_parser_create(void) { return new (std::nothrow) mi355x_h264_parser(); }
void mi355x_h264_parser_destroy(mi355x_h264_parser* p) { delete p; }
int mi355x_h264_parser_parse(mi355x_h264_parser* p, const uint8_t* au, size_t len)
{
    if (!p || !au) return -1;
    try {
        return p->p.parse_access_unit(au, len);
    } catch (const std::exception& ex) {   // (allocation failure of a per-macroblock array: reported, never thrown through the C ABI)
        p->p.lose_refs();
        p->p.set_error(std::string("out of memory: ") + ex.what());
        return -1;
    }
}
const char* mi355x_h264_parser_error(const mi355x_h264_parser* p) { return p ? p->p.error().c_str() : "no parser"; }
int mi355x_h264_parser_info(const mi355x_h264_parser* p, int32_t* out, int n)
{
    if (!p || !out || n < 12) return -1;
    const h264dec::Picture& c = p->p.picture();
    const int32_t v[21] = {c.mbw, c.mbh, c.width, c.height, c.idr, c.qp, c.slice_rows, c.deblock_idc, c.num_ref_active, c.t8x8_mode, c.has_pcm, c.has_intra | (c.has_inter << 1),
                           c.cqo[0], c.cqo[1], c.filter_oa, c.filter_ob, c.one_qp, c.ref_age[0], c.ref_age[1], c.ref_age[2], c.is_ref};
    const int m = n < 17 ? 12 : (n < 20 ? 17 : (n < 21 ? 20 : 21));   // (a caller with an earlier layout's slots gets those)
    memcpy(out, v, (size_t)m * sizeof(int32_t));
    return m;
}
int mi355x_h264_parser_set_loss_mode(mi355x_h264_parser* p, int mode)
{
    if (!p || mode < MI355X_H264_LOSS_STRICT || mode > MI355X_H264_LOSS_CONCEAL) return MI355X_H264_E_ARG;
    p->p.set_conceal(mode == MI355X_H264_LOSS_CONCEAL);
    return MI355X_H264_OK;
}
int mi355x_h264_parser_loss(const mi355x_h264_parser* p, int32_t* out)
{
    if (!p || !out) return MI355X_H264_E_ARG;
    const h264dec::Picture& c = p->p.picture();
    out[0] = c.nconcealed; out[1] = c.gap; out[2] = c.joined ? 1 : 0; out[3] = c.recovery; out[4] = p->p.lost() ? 1 : 0;
    return MI355X_H264_OK;
}
int mi355x_h264_parser_colour(const mi355x_h264_parser* p, int32_t* out, int n)
{
    if (!p || !out || n < 8) return -1;
    const h264dec::Vui& v = p->p.sps().vui;
    vui_report(v, out);
    if (n < 10) return 8;
    out[8] = v.present ? 1 : 0; out[9] = v.dec_buffering;
    return 10;
}
// what: 0 MbInfo (32 B / macroblock), 1 quadrant vectors (16 B), 2 Intra4x4 modes (16 B), 3 levels (832 B)
int64_t mi355x_h264_parser_read(const mi355x_h264_parser* p, int what, void* dst, size_t cap)
{
    if (!p || !dst) return -1;
    const h264dec::Picture& c = p->p.picture();
    const void* src = nullptr;
    size_t n = 0;
    switch (what) {
        case 0: src = c.mb.data(); n = c.mb.size() * sizeof(h264dec::MbRec); break;
        case 1: src = c.mvq.data(); n = c.mvq.size() * sizeof(int16_t); break;
        case 2: src = c.aux.data(); n = c.aux.size(); break;
        case 3: {   // the level lists as int16 (what k_dec_widen_pos + k_dec_patch make of levels8 + big on the GPU)
            n = c.levels8.size() * sizeof(int16_t);
            if (cap < n) return -1;
            int16_t* o = (int16_t*)dst;
            for (size_t m = 0; m < c.mb.size(); m++) {
                const int8_t* s8 = c.levels8.data() + m * h264dec::L_STRIDE;
                int16_t* d16 = o + m * h264dec::L_STRIDE;
                if (c.mb[m].type == h264dec::T_IPCM) { memset(d16, 0, h264dec::L_STRIDE * sizeof(int16_t)); memcpy(d16, s8, 384); }
                else for (int k = 0; k < h264dec::L_STRIDE; k++) d16[k] = s8[k];
            }
            for (const auto& b : c.big) o[b.idx] = (int16_t)b.val;
            return (int64_t)n;
        }
        case 4: src = c.mbqp.data(); n = c.mbqp.size(); break;
        case 5: src = c.mv4.data(); n = c.mv4.size() * sizeof(int16_t); break;
        case 6: src = c.refq.data(); n = c.refq.size(); break;
        case 7: src = c.mbavail.data(); n = c.mbavail.size(); break;
        case 8: src = c.concealed.data(); n = c.concealed.size(); break;
        default: return -1;
    }
    if (cap < n) return -1;
    memcpy(dst, src, n);
    return (int64_t)n;
}

}  // extern "C"
