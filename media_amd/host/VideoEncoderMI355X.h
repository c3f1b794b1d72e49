/*
 * media_amd/host/VideoEncoderMI355X.h -- the MI355X backend of the VideoEncoder plugin surface, a peer of the
 * reference's OpenH264 adapter (/root/reference/video_codec/VideoEncoderOpenH264.h:27-196).  The shared wrapper
 * behaviour lives in PropertyDrivenEncoder; the engine here is the HIP encode path behind the C ABI of
 * include/mi355x_h264.h, plus the two pieces of host logic OpenH264 keeps inside its library: frame-level rate
 * control for the bitrate mode and the scene-change IDR.
 */
#ifndef VIDEO_ENCODER_MI355X_H
#define VIDEO_ENCODER_MI355X_H

#include <vector>

#include "PropertyDrivenEncoder.h"
#include "mi355x_h264.h"

class VideoEncoderMI355X : public PropertyDrivenEncoder {
public:
    struct Rc {
        static constexpr int32_t kQpMin = 12, kQpMax = 48, kQpStart = 30;  // rate-control range
        static constexpr uint32_t kSceneCutCostPerMb = 3000;               // mean motion cost that triggers an IDR
    };

    VideoEncoderMI355X();
    ~VideoEncoderMI355X() override;

    // test hooks
    int32_t LastFrameQp() const { return m_lastQp; }
    uint32_t SceneCuts() const { return m_sceneCuts; }
    // quality report of the last picture that went out (extension key persist.vmi.video.encode.psnr = 1; after a scene-change
    // re-code: of the IDR picture).  false: the key is off or there has been no picture
    bool LastFrameQuality(mi355x_h264_quality *out) const;
    // its SSIM record (extension key persist.vmi.video.encode.ssim = 1).  false: the key is off or there is no record
    bool LastFrameSsim(mi355x_h264_ssim *out) const;
    // measurement hook (bench.py reads the reconstruction for PSNR): luma reconstruction of the last picture, coded size
    int64_t ReadReconY(void *dst, size_t cap, int32_t *codedWidth, int32_t *codedHeight);
    bool Shared() const { return m_stream != nullptr; }
    // extension keys persist.vmi.video.encode.input / .inputmem: "nv12" / "rgba" -> MI355X_H264_INPUT_NV12 / _RGBA, anything else
    // (or unset) -> MI355X_H264_INPUT_I420, the reference's videoFormatI420; "device" -> true, anything else -> host memory
    static int32_t ParseInputLayout(const std::string &value);
    static bool ParseInputDevice(const std::string &value);
    // extension key persist.vmi.video.encode.refs: "2" / "3" -> that many reference pictures; anything else (or unset) -> 1, the
    // reference preset's iNumRefFrame
    static int32_t ParseRefs(const std::string &value);
    // extension key persist.vmi.video.encode.psnr: "1" -> the library's quality report is on (include/mi355x_h264.h, "quality
    // report"), on the stream path and with an engine of its own alike; anything else (or unset) -> off
    static bool ParsePsnr(const std::string &value);
    // extension key persist.vmi.video.encode.ssim: "1" -> the quality report is on with both metrics (SSE and SSIM), with or
    // without .psnr, on both paths; anything else (or unset) -> what .psnr says
    static bool ParseSsim(const std::string &value);
    // extension keys persist.vmi.video.encode.srcwidth / .srcheight: EncodeOneFrame takes pictures of that size and the device
    // resamples them to the coded size (include/mi355x_h264.h, "scaled streams").  1: both are decimal numbers, even, 16 .. 4096,
    // at least the coded size and at most 4 times it (*srcWidth, *srcHeight set); 0: neither key is set; -1: anything else (one
    // key alone, junk, out of range) - the reference's behaviour, with one WARN line
    static int ParseSourceSize(const std::string &width, const std::string &height, uint32_t codedWidth, uint32_t codedHeight,
                               int32_t *srcWidth, int32_t *srcHeight);

    // extension keys persist.vmi.video.encode.colour ("bt601" | "bt709") and .range ("limited" | "full"): either key present and
    // valid describes the stream (include/mi355x_h264.h, "colour description"), the other defaulting to bt601 / limited.  1: *out is
    // the description; 0: neither key is set (no description, the reference's behaviour); -1: a key holds anything else - the
    // reference's behaviour, with one WARN line
    static int ParseColour(const std::string &colour, const std::string &range, mi355x_h264_colour *out);
    // the description the engine was opened with (false: none)
    bool Colour(mi355x_h264_colour *out) const;
    // extension key persist.vmi.video.encode.temporallayers: "2" -> two temporal layers, every second P picture a non-reference
    // picture a forwarder may drop (include/mi355x_h264.h, "temporal layers"), on both paths; unset or "1" -> 1, the reference
    // preset's iTemporalLayerNum; anything else -> 1 with *junk set (the reference's behaviour, with one WARN line).  The rate
    // controller sees every picture as it does with one layer
    static int32_t ParseTemporalLayers(const std::string &value, bool *junk);
    // temporal layer (0 / 1) of the last picture that went out; -1 before the first
    int32_t LastTemporalId() const { return m_lastTemporalId; }
    // extension key persist.vmi.video.encode.intrarefresh: "n" (decimal, 2..32) -> intra refresh over n slice bands, which sets
    // slices = n (include/mi355x_h264.h, "intra refresh"), on both paths; unset -> 0, off.  Anything else, a picture of `height`
    // that has no n bands of two macroblock rows, a .slices of another count (slices: the parsed key, 0 unset), refs > 1 or two
    // temporal layers -> 0 with *warn set (one WARN line, the stream the other keys describe)
    static int32_t ParseIntraRefresh(const std::string &value, int32_t slices, int32_t refs, int32_t layers, uint32_t height, bool *warn);
    // the all-intra band of the last picture that went out; -1 for an IDR picture, with refresh off and before the first
    int32_t LastRefreshBand() const { return m_lastRefreshBand; }
    // extension key persist.vmi.video.encode.damage: "detect" -> every host picture goes through the damage call of its layout with
    // MI355X_H264_DAMAGE_DETECT (include/mi355x_h264.h, "damage tiles": only the tiles that changed are transferred, the bytes of
    // the stream are the same); "off", unset or empty -> 0, whole pictures; anything else -> -1: one WARN line, "off" is written
    // back to the key and whole pictures go.  An engine of its own (.shared = 0) and pictures in device memory (.inputmem = device)
    // have no staging slot to patch: whole pictures (device: none) go as before and one INFO line says so
    static int32_t ParseDamage(const std::string &value);
    // The rectangles of the NEXT EncodeOneFrame only, in luma samples of the picture that call is handed: it goes through the damage
    // call with them (n = 0: nothing changed), whatever the key says; a scene-change re-code of that picture takes them again.  The
    // picture that is encoded is the previous one with the tiles the rectangles touch replaced - rectangles that miss a change
    // are the caller's affair.  false: n < 0, n > 0 without rectangles or a negative width / height - nothing was set.  On a path
    // that cannot use damage the next picture goes whole and one INFO line says so
    using Rect = mi355x_h264_rect;
    bool SetNextDamage(const Rect *rects, int n);
    // test hook: mi355x_h264_stream_last_upload of the object's stream; false with an engine of its own
    bool LastUpload(uint64_t *bytes, uint32_t *tiles, uint32_t *tilesTotal, int *mode) const;

protected:
    const char *BackendName() const override { return "MI355X HIP"; }
    bool EngineOpen(const Settings &s) override;
    void EngineClose() override;
    bool EngineReady() const override { return m_engine != nullptr || m_stream != nullptr; }
    bool EngineEncode(const uint8_t *i420, uint8_t **out, uint32_t *outLen) override;
    bool EngineForceIdr() override;
    uint32_t EnginePictureBytes() const override { return m_input == MI355X_H264_INPUT_RGBA ? SrcLumaBytes() * 4 : SrcLumaBytes() * 3 / 2; }

private:
    // the size of the pictures EncodeOneFrame is handed: the source size of a scaled stream, else the coded size
    uint32_t SrcWidth() const { return m_srcWidth > 0 ? static_cast<uint32_t>(m_srcWidth) : Active().width; }
    uint32_t SrcLumaBytes() const { return m_srcWidth > 0 ? static_cast<uint32_t>(m_srcWidth) * static_cast<uint32_t>(m_srcHeight) : LumaBytes(); }
    int EncodePicture(const uint8_t *i420, uint8_t **out, uint32_t *outLen, int *frameType);
    void RateControlUpdate(uint32_t frameBytes, bool isIdr);
    static int32_t StartQp(uint32_t bitrate, uint32_t fps, uint32_t width, uint32_t height);
    void QualityAfterPicture(bool isIdr);
    void QualityLogGop();

    mi355x_h264_encoder *m_engine = nullptr;   // an engine of its own (persist.vmi.video.encode.shared = 0), or
    mi355x_h264_stream *m_stream = nullptr;    // a stream of the process-wide shared engine (the default)
    // rate control (the reference preset runs RC_BITRATE_MODE, VideoEncoderOpenH264.cpp:274)
    int32_t m_fixedQp = -1;            // >= 0: extension property persist.vmi.video.encode.qp selects fixed QP
    int32_t m_qp = Rc::kQpStart, m_lastQp = 0;
    int64_t m_bufferBits = 0;          // virtual buffer fullness relative to the target rate
    int64_t m_gopLeft = 0, m_picsLeft = 0, m_meanP = 0;   // GOP budget left, P pictures left in the GOP, running mean of the P pictures' bits
    bool m_sceneDetect = true;         // bEnableSceneChangeDetect = 1 in the reference preset (ref :283)
    uint32_t m_sceneCuts = 0;
    int32_t m_input = MI355X_H264_INPUT_I420;   // layout of the pictures EncodeOneFrame is handed (persist.vmi.video.encode.input)
    int32_t m_srcWidth = 0, m_srcHeight = 0;    // > 0: the pictures' size (.srcwidth / .srcheight), resampled to the coded size on the device
    bool m_inputDevice = false;                 // inputData is an address in the object's device's memory (.inputmem = device)
    int32_t m_intraRefresh = 0, m_lastRefreshBand = -1;     // .intrarefresh (bands, 0 off); the band of the last picture that went out
    bool m_damageDetect = false, m_haveNextDamage = false, m_damageInfoSaid = false;   // .damage = detect; SetNextDamage holds for one picture
    std::vector<mi355x_h264_rect> m_nextDamage;
    int32_t m_temporalLayers = 1, m_lastTemporalId = -1;   // .temporallayers; the layer of the last picture that went out
    // quality report (persist.vmi.video.encode.psnr = 1): the last picture's record and the sums of the GOP being coded
    bool m_psnr = false, m_haveQuality = false;
    mi355x_h264_quality m_lastQuality{};
    // SSIM beside it (persist.vmi.video.encode.ssim = 1)
    bool m_ssim = false, m_haveSsim = false;
    mi355x_h264_ssim m_lastSsim{};
    int64_t m_gopSsimSum[3] = {0, 0, 0};
    uint64_t m_gopSsimWindows[3] = {0, 0, 0};
    uint32_t m_gopSsimPictures = 0;
    uint64_t m_gopSse[3] = {0, 0, 0}, m_gopSamples[3] = {0, 0, 0}, m_gopBytes = 0;
    uint32_t m_gopPictures = 0;
};

#endif  // VIDEO_ENCODER_MI355X_H
