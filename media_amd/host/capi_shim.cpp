// media_amd/host/capi_shim.cpp -- flat C entry points over the C++ plugin surface so
// that the Python tests can drive CreateVideoEncoder / VideoEncoder exactly as the
// (unseen) VMI caller would: Create -> Init -> Start -> Encode x N -> Stop -> Destroy.
#include <cstring>
#include "MediaLog.h"
#include "Property.h"
#include "VideoCodecApi.h"
#include "VideoEncoderMI355X.h"
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-function"
#include "../csrc/host_framing.h"   // PicSeq (plain C++): vc_debug_ref_counts
#pragma GCC diagnostic pop

extern "C" {
uint32_t vc_create(void **enc) { return CreateVideoEncoder(reinterpret_cast<VideoEncoder **>(enc)); }
uint32_t vc_delete(void *enc) { return DestroyVideoEncoder(static_cast<VideoEncoder *>(enc)); }
uint32_t vc_init(void *enc) { return static_cast<VideoEncoder *>(enc)->InitEncoder(); }
uint32_t vc_start(void *enc) { return static_cast<VideoEncoder *>(enc)->StartEncoder(); }
uint32_t vc_encode(void *enc, const uint8_t *in, uint32_t inSize, uint8_t **out, uint32_t *outSize)
{
    return static_cast<VideoEncoder *>(enc)->EncodeOneFrame(in, inSize, out, outSize);
}
// inputData as an address (persist.vmi.video.encode.inputmem = device: a picture in device memory)
uint32_t vc_encode_addr(void *enc, uint64_t addr, uint32_t inSize, uint8_t **out, uint32_t *outSize)
{
    return static_cast<VideoEncoder *>(enc)->EncodeOneFrame(reinterpret_cast<const uint8_t *>(static_cast<uintptr_t>(addr)), inSize, out, outSize);
}
// how the two input extension keys read a value (host logic, no device)
int32_t vc_parse_input_layout(const char *value) { return VideoEncoderMI355X::ParseInputLayout(value != nullptr ? value : ""); }
int32_t vc_parse_input_device(const char *value) { return VideoEncoderMI355X::ParseInputDevice(value != nullptr ? value : "") ? 1 : 0; }
// persist.vmi.video.encode.srcwidth / .srcheight at a coded size: 1 (and the size), 0 (neither set) or -1 (rejected)
int32_t vc_parse_source_size(const char *width, const char *height, uint32_t codedWidth, uint32_t codedHeight, int32_t *srcWidth, int32_t *srcHeight)
{
    return VideoEncoderMI355X::ParseSourceSize(width != nullptr ? width : "", height != nullptr ? height : "", codedWidth, codedHeight, srcWidth, srcHeight);
}
// persist.vmi.video.encode.refs: 2 or 3 are taken, anything else is one reference picture
// persist.vmi.video.encode.temporallayers: 1 or 2; *junk = the value is none the key takes (one WARN line, one layer)
int32_t vc_parse_temporal_layers(const char *value, int32_t *junk)
{
    bool j = false;
    const int32_t n = VideoEncoderMI355X::ParseTemporalLayers(value != nullptr ? value : "", &j);
    if (junk != nullptr) *junk = j ? 1 : 0;
    return n;
}
// persist.vmi.video.encode.intrarefresh: the bands (0: off); *warn = junk or a conflict with the other keys (one WARN line)
int32_t vc_parse_intra_refresh(const char *value, int32_t slices, int32_t refs, int32_t layers, uint32_t height, int32_t *warn)
{
    bool w = false;
    const int32_t n = VideoEncoderMI355X::ParseIntraRefresh(value != nullptr ? value : "", slices, refs, layers, height, &w);
    if (warn != nullptr) *warn = w ? 1 : 0;
    return n;
}
int32_t vc_last_refresh_band(void *enc)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr ? m->LastRefreshBand() : -1;
}
// persist.vmi.video.encode.damage: 1 detect, 0 off / unset, -1 rejected (one WARN line, "off" written back)
int32_t vc_parse_damage(const char *value) { return VideoEncoderMI355X::ParseDamage(value != nullptr ? value : ""); }
// VideoEncoderMI355X::SetNextDamage; rects = n * {x, y, w, h} int32.  1: set, 0: refused, -1: not this backend
int32_t vc_set_next_damage(void *enc, const int32_t *rects, int32_t n)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    if (m == nullptr) return -1;
    return m->SetNextDamage(reinterpret_cast<const VideoEncoderMI355X::Rect *>(rects), n) ? 1 : 0;
}
// VideoEncoderMI355X::LastUpload: 0 (and the four values) or -1 (an engine of its own)
int32_t vc_last_upload(void *enc, uint64_t *bytes, uint32_t *tiles, uint32_t *tilesTotal, int32_t *mode)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    int md = 0;
    if (m == nullptr || !m->LastUpload(bytes, tiles, tilesTotal, &md)) return -1;
    *mode = md;
    return 0;
}
int32_t vc_last_temporal_id(void *enc)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr ? m->LastTemporalId() : -1;
}
int32_t vc_parse_refs(const char *value) { return VideoEncoderMI355X::ParseRefs(value != nullptr ? value : ""); }
// persist.vmi.video.encode.psnr: "1" turns the quality report on, anything else leaves it off
int32_t vc_parse_psnr(const char *value) { return VideoEncoderMI355X::ParsePsnr(value != nullptr ? value : "") ? 1 : 0; }
// persist.vmi.video.encode.ssim: "1" turns the quality report on with both metrics, anything else leaves it as .psnr says
int32_t vc_parse_ssim(const char *value) { return VideoEncoderMI355X::ParseSsim(value != nullptr ? value : "") ? 1 : 0; }
// the library's own rules (host_framing.h, shared with the engine): is `metrics` a value mi355x_h264_quality_enable_ex takes, and
// what MI355X_H264_QUALITY = value turns on when an engine is created (MI355X_H264_QUALITY_* bits)
int32_t vc_debug_quality_metrics_ok(uint32_t metrics) { return quality_metrics_ok(metrics) ? 1 : 0; }
uint32_t vc_debug_quality_env(const char *value) { return quality_env_metrics(value); }
// persist.vmi.video.encode.colour / .range: 1 (and matrix, full_range), 0 (neither set) or -1 (rejected)
int32_t vc_parse_colour(const char *colour, const char *range, int32_t *matrix, int32_t *fullRange)
{
    mi355x_h264_colour c{};
    const int rc = VideoEncoderMI355X::ParseColour(colour != nullptr ? colour : "", range != nullptr ? range : "", &c);
    if (rc > 0) { *matrix = c.matrix; *fullRange = c.full_range; }
    return rc;
}
// the description the object's engine was opened with: 1 (and matrix, full_range) or 0
int32_t vc_colour(void *enc, int32_t *matrix, int32_t *fullRange)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    mi355x_h264_colour c{};
    if (m == nullptr || !m->Colour(&c)) return 0;
    *matrix = c.matrix; *fullRange = c.full_range;
    return 1;
}
// The parameter sets (Annex-B SPS + PPS) the library writes for a stream shape, from the host code alone (host_framing.h,
// build_parameter_sets): shape = the fourteen fields of StreamShape in order.  Returns the bytes, or -1 when cap is too small
int32_t vc_debug_parameter_sets(const int32_t *shape, uint8_t *dst, int32_t cap)
{
    const StreamShape f{shape[0], shape[1], shape[2], shape[3], shape[4], shape[5], shape[6], shape[7], shape[8], shape[9], shape[10], shape[11], shape[12], shape[13], 0};
    const std::vector<uint8_t> ps = build_parameter_sets(f);
    if (static_cast<size_t>(cap) < ps.size()) return -1;
    std::memcpy(dst, ps.data(), ps.size());
    return static_cast<int32_t>(ps.size());
}
// level_idc the library picks for a picture of mbs macroblocks at fps (host_framing.h, pick_level; never below 3.2)
int32_t vc_debug_level(int32_t mbs, int32_t fps) { return std::max(32, pick_level(mbs, fps)); }
// The one rule for a picture's number of reference pictures (PicSeq::avail_refs, shared by the engine and the stream hub), driven
// as both drive it: n pictures of a stream that searches nrefs pictures with an IDR every gop; force[i] != 0 forces an IDR at
// picture i.  out[i] = the count of picture i (0: an IDR picture).
void vc_debug_ref_counts(int32_t nrefs, int32_t gop, const uint8_t *force, int32_t n, int32_t *out)
{
    PicSeq seq;
    for (int32_t i = 0; i < n; i++) {
        if (force != nullptr && force[i] != 0) seq.force_idr = 1;
        const bool idr = seq.next_is_idr(gop);
        seq.begin(idr);
        out[i] = seq.avail_refs(idr, nrefs);
        seq.advance(idr, nrefs + 1, 1);
    }
}
uint32_t vc_stop(void *enc) { return static_cast<VideoEncoder *>(enc)->StopEncoder(); }
void vc_destroy(void *enc) { static_cast<VideoEncoder *>(enc)->DestroyEncoder(); }
uint32_t vc_reset(void *enc) { return static_cast<VideoEncoder *>(enc)->ResetEncoder(); }
int32_t vc_last_qp(void *enc)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr ? m->LastFrameQp() : -1;
}
// the quality record (mi355x_h264_quality) of the last picture that went out; 0, or -1 when there is none
int32_t vc_last_quality(void *enc, mi355x_h264_quality *out)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr && m->LastFrameQuality(out) ? 0 : -1;
}
// the SSIM record (mi355x_h264_ssim) of the last picture that went out (persist.vmi.video.encode.ssim = 1); 0, or -1 when there is none
int32_t vc_last_ssim(void *enc, mi355x_h264_ssim *out)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr && m->LastFrameSsim(out) ? 0 : -1;
}
uint32_t vc_scene_cuts(void *enc)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    return m != nullptr ? m->SceneCuts() : 0;
}
// copies the luma reconstruction of the last picture (coded size) into dst; returns bytes or < 0 (measurement hook: PSNR)
int64_t vc_debug_recon_y(void *enc, void *dst, uint64_t cap, int32_t *codedWidth, int32_t *codedHeight)
{
    auto *m = dynamic_cast<VideoEncoderMI355X *>(static_cast<VideoEncoder *>(enc));
    if (m == nullptr) return -1;
    return m->ReadReconY(dst, static_cast<size_t>(cap), codedWidth, codedHeight);
}
void vc_prop_set(const char *key, const char *value) { SetEncParam(key, value); }
int32_t vc_prop_get_int(const char *key) { return GetIntEncParam(key); }
int32_t vc_prop_get_str(const char *key, char *buf, int32_t cap)
{
    const std::string v = GetStrEncParam(key);
    if (cap <= 0) return -1;
    std::strncpy(buf, v.c_str(), static_cast<size_t>(cap) - 1);
    buf[cap - 1] = 0;
    return static_cast<int32_t>(v.size());
}
}
