/*
 * media_amd/host/VideoDecoderMI355X.h -- H.264 decoder backend for the VideoDecoder plugin surface, a peer of the reference's
 * NETINT adapter (/root/reference/video_decoder/VideoDecoderNetint.h:13-31).  Same operator API and the same observable
 * behaviour at the surface (stop state, picture-size change event, copy hook); the engine beneath is the C ABI of
 * include/mi355x_h264_dec.h: host CAVLC parser + reconstruction on the MI355X.
 */
#ifndef VIDEO_DECODER_MI355X_H
#define VIDEO_DECODER_MI355X_H

#include <string>
#include <vector>
#include "VideoDecoder.h"
#include "mi355x_h264_dec.h"

class VideoDecoderMI355X : public VideoDecoder {
public:
    VideoDecoderMI355X() = default;
    ~VideoDecoderMI355X() override;

    DecoderRetCode CreateDecoder(MediaStreamFormat decType) override;
    DecoderRetCode InitDecoder() override;
    DecoderRetCode SetDecodeParams(DecodeParamsIndex index, void *decParams) override;
    DecoderRetCode GetDecodeParams(DecodeParamsIndex index, void *decParams) override;
    DecoderRetCode SetCallbacks(std::function<void(DecodeEventIndex, uint32_t, void *)> eventCallBack) override;
    DecoderRetCode SetCopyFrameFunc(
        std::function<uint32_t(uint8_t*, uint8_t*, const PicInfoParams &, uint32_t)> copyFrame) override;
    DecoderRetCode SendStreamData(uint8_t *buffer, uint32_t filledLen) override;
    DecoderRetCode RetrieveFrameData(uint8_t *buffer, uint32_t maxLen, uint32_t *filledLen) override;
    DecoderRetCode Flush() override;
    DecoderRetCode StartDecoder() override;
    DecoderRetCode StopDecoder() override;
    void DestroyDecoder() override;

    // test hooks
    uint64_t PicturesDecoded() const { return m_pictures; }
    // what the sequence parameter set of the last picture says (out[8] of mi355x_h264_dec_colour), and how often it has changed
    // since StartDecoder (the first picture counts: 1)
    uint32_t ColourChanges(int32_t out[8]) const;
    // extension keys persist.vmi.video.decode.outwidth / .outheight: frames are delivered at that size, resampled on the device
    // (include/mi355x_h264_dec.h, "output size").  Both decimal, even and 2..4096: 1 and the size; neither set: 0; anything else
    // (one key alone, junk): -1, and the caller keeps the native size.  Parsed as VideoEncoderMI355X parses .srcwidth / .srcheight
    static int ParseOutputSize(const std::string &width, const std::string &height, int32_t *outWidth, int32_t *outHeight);
    // extension key persist.vmi.video.decode.lossmode: 0 strict (the default), 1 conceal (include/mi355x_h264_dec.h, "loss mode").
    // Returns 1 (and the mode), 0 (not set) or -1 (rejected: anything but "0" and "1")
    static int ParseLossMode(const std::string &value, int32_t *mode);
    bool Inexact() const { return m_inexact; }   // conceal mode: the last picture may differ from the lossless decode

private:
    static constexpr uint32_t kDefaultWidth = 1280, kDefaultHeight = 720;   // the reference adapter's defaults (VideoDecoderNetint.h:34-35)

    mi355x_h264_decoder *m_engine = nullptr;
    bool m_created = false, m_stop = true, m_pending = false;
    uint32_t m_writeWidth = kDefaultWidth, m_writeHeight = kDefaultHeight;
    int32_t m_stride = static_cast<int32_t>(kDefaultWidth);
    uint64_t m_pictures = 0;
    std::vector<uint8_t> m_frame;   // the waiting picture, tight I420 - or tight RGBA, when the out port was set to PIXEL_FORMAT_RGBA_8888
    // the out port's format: PIXEL_FORMAT_YUV_420P (the default) or PIXEL_FORMAT_RGBA_8888 (SetDecodeParams, INDEX_PORT_FORMAT_INFO).
    // RGBA follows the stream's colour description (include/mi355x_h264_dec.h, "colour")
    int32_t m_outFormat = PIXEL_FORMAT_YUV_420P;
    int32_t m_colour[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t m_colourChanges = 0;
    uint32_t m_frameWidth = 0, m_frameHeight = 0;   // of the waiting picture as delivered
    int32_t m_lossMode = 0;                        // the loss mode asked for with .lossmode (read by StartDecoder)
    bool m_inexact = false;                        // the last picture had tainted macroblocks: one INFO line when that ends
    int32_t m_outWidth = 0, m_outHeight = 0;       // > 0: the size asked for with .outwidth / .outheight (read by StartDecoder)
    uint32_t m_nativeWarnWidth = 0, m_nativeWarnHeight = 0;   // the native size the last "cannot be resampled" WARN line named
    void ReadOutputSizeKeys();
    void ReadLossModeKey();
    std::function<void(DecodeEventIndex, uint32_t, void *)> m_eventCallBack;
    std::function<uint32_t(uint8_t*, uint8_t*, const PicInfoParams &, uint32_t)> m_copyFrame;
};

#endif
