// media_amd/host/VideoEncoderMI355X.cpp -- see VideoEncoderMI355X.h.
#define LOG_TAG "VideoEncoderMI355X"
#include "VideoEncoderMI355X.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include "MediaLog.h"
#include "Property.h"
#include "../csrc/damage.h"   // the key's parser (plain C++)

namespace {
bool Within(int32_t v, int32_t lo, int32_t hi) { return v >= lo && v <= hi; }
int ProfileIdc(const std::string &name) { return name == "high" ? 100 : (name == "main" ? 77 : 66); }
}  // namespace

VideoEncoderMI355X::VideoEncoderMI355X() { INFO("MI355X encoder object created"); }

VideoEncoderMI355X::~VideoEncoderMI355X()
{
    EngineClose();
    INFO("MI355X encoder object gone");
}

bool VideoEncoderMI355X::EngineOpen(const Settings &s)
{
    // the preset of InitParams / InitParamExt (ref :228-296) in the C ABI's terms: one layer, one slice per
    // picture, one reference frame, loop filter on, CAVLC, IDR every gop pictures
    if (((s.width | s.height) & 1u) != 0) {   // 4:2:0: the chroma planes are (width / 2) x (height / 2)
        ERR("picture size %ux%u: width and height must be even", s.width, s.height);
        return false;
    }
    mi355x_h264_config cfg;
    mi355x_h264_default_config(&cfg);
    cfg.width = static_cast<int32_t>(s.width);
    cfg.height = static_cast<int32_t>(s.height);
    cfg.fps = static_cast<int32_t>(s.fps);
    cfg.bitrate = static_cast<int32_t>(s.bitrate);
    cfg.gop = static_cast<int32_t>(s.gop);
    cfg.profile_idc = ProfileIdc(s.profile);
    if (cfg.profile_idc != 66) {
        // the reference preset asks for CABAC (iEntropyCodingModeFlag = 1, ref :291); this engine codes CAVLC in every profile
        INFO("profile_idc %d is coded with CAVLC (entropy_coding_mode_flag = 0): CABAC is not built", cfg.profile_idc);
    }
    cfg.disable_deblock = 0;
    cfg.batch = 1;
    cfg.device = std::max(0, GetIntEncParam("persist.vmi.video.encode.device"));
    // extension keys: a valid QP selects fixed-QP coding instead of the preset's
    // bitrate mode; "0" switches the scene-change IDR off
    const int32_t qp = GetIntEncParam("persist.vmi.video.encode.qp");
    m_fixedQp = Within(qp, 10, 51) ? qp : -1;
    cfg.rc_mode = m_fixedQp >= 0 ? MI355X_H264_RC_FIXED_QP : MI355X_H264_RC_BITRATE;
    cfg.qp = m_fixedQp >= 0 ? m_fixedQp : StartQp(s.bitrate, s.fps, s.width, s.height);
    m_qp = cfg.qp;
    m_bufferBits = 0;
    m_gopLeft = 0;
    m_picsLeft = 0;
    m_meanP = 0;
    m_sceneDetect = GetStrEncParam("persist.vmi.video.encode.scenedetect") != "0";
    // extension: 2..64 slice bands per picture for a shorter per-picture latency; anything else keeps the preset's
    // single slice (SM_SINGLE_SLICE, ref :247)
    const int32_t slices = GetIntEncParam("persist.vmi.video.encode.slices");
    cfg.slices = Within(slices, 2, 64) ? slices : 0;
    // extension: "0" = exhaustive integer motion search instead of the default seeded one (include/mi355x_h264.h config.search)
    if (GetStrEncParam("persist.vmi.video.encode.search") == "0") {
        cfg.search = MI355X_H264_SEARCH_EXHAUSTIVE;
    }
    // extensions: the layout of the pictures ("nv12", "rgba"; else the reference's tight I420) and where they lie ("device":
    // inputData is an address in this device's memory, read in place; else host memory).  include/mi355x_h264.h, "streams"
    m_input = ParseInputLayout(GetStrEncParam("persist.vmi.video.encode.input"));
    m_inputDevice = ParseInputDevice(GetStrEncParam("persist.vmi.video.encode.inputmem"));
    // extension: "2" / "3" = that many reference pictures are searched and ref_idx_l0 is coded; anything else keeps the preset's
    // one (iNumRefFrame = 1, ref :290).  Both paths below honour it
    cfg.refs = ParseRefs(GetStrEncParam("persist.vmi.video.encode.refs"));
    // extension: "1" = the library compares every picture with its source (SSE per plane; include/mi355x_h264.h, "quality report"):
    // LastFrameQuality() and one log line per GOP.  The switch of a shared engine holds for all its streams and ends with it:
    // an object without the key leaves it as it finds it and reads nothing
    m_psnr = ParsePsnr(GetStrEncParam("persist.vmi.video.encode.psnr"));
    // extension: "1" = the report is on with both metrics, SSIM beside the SSE ("quality report: SSIM"), with or without .psnr:
    // LastFrameSsim() and a log line of its own per GOP.  (An object with .psnr alone that opens a stream of the same shared
    // engine later sets the switch to the SSE alone for all of them; this object then reads no SSIM record and writes no line.)
    m_ssim = ParseSsim(GetStrEncParam("persist.vmi.video.encode.ssim"));
    m_haveQuality = m_haveSsim = false;
    m_gopPictures = 0;
    m_gopSsimPictures = 0;
    const unsigned metrics = m_ssim ? (MI355X_H264_QUALITY_SSE | MI355X_H264_QUALITY_SSIM) : MI355X_H264_QUALITY_SSE;
    // One engine per object (mi355x_h264_create) costs every picture its own launch sequence.  The default is a STREAM of the
    // shared engine: the pictures that the encoder objects of one process hand over at about the same time are coded in one
    // lockstep step (include/mi355x_h264.h, "streams"; same bitstream).  persist.vmi.video.encode.shared = 0 (or the environment
    // variable MI355X_H264_HUB=0) keeps the engine of its own.
    const char *hubEnv = getenv("MI355X_H264_HUB");
    const bool shared = GetStrEncParam("persist.vmi.video.encode.shared") != "0" && !(hubEnv != nullptr && hubEnv[0] == '0');
    // extension: pictures of srcwidth x srcheight, resampled to the coded size on the device (stream path only)
    const std::string srcW = GetStrEncParam("persist.vmi.video.encode.srcwidth"), srcH = GetStrEncParam("persist.vmi.video.encode.srcheight");
    m_srcWidth = m_srcHeight = 0;
    const int haveSrc = ParseSourceSize(srcW, srcH, s.width, s.height, &m_srcWidth, &m_srcHeight);
    if (haveSrc < 0) {
        WARN("source size [%s] x [%s] rejected for %ux%u: pictures are taken at the coded size", srcW.c_str(), srcH.c_str(), s.width, s.height);
    }
    if (haveSrc > 0 && !shared) {
        ERR("source size %dx%d: scaling exists on the stream path only (persist.vmi.video.encode.shared = 0 is set)", m_srcWidth, m_srcHeight);
        m_srcWidth = m_srcHeight = 0;
        return false;
    }
    // extension: matrix and range of the stream's samples, written into the SPS; RGBA pictures are converted with them.  Both paths
    const std::string colourKey = GetStrEncParam("persist.vmi.video.encode.colour"), rangeKey = GetStrEncParam("persist.vmi.video.encode.range");
    mi355x_h264_colour colour{};
    const int haveColour = ParseColour(colourKey, rangeKey, &colour);
    if (haveColour < 0) {
        WARN("colour [%s] / range [%s] rejected: the stream carries no colour description", colourKey.c_str(), rangeKey.c_str());
    }
    // extension: "2" = two temporal layers, the odd pictures of a GOP non-reference and droppable.  Both paths
    const std::string layersKey = GetStrEncParam("persist.vmi.video.encode.temporallayers");
    bool layersJunk = false;
    m_temporalLayers = ParseTemporalLayers(layersKey, &layersJunk);
    m_lastTemporalId = -1;
    if (layersJunk) {
        WARN("temporal layers [%s] rejected: one layer", layersKey.c_str());
    }
    // extension: "n" (2..32) = intra refresh over n slice bands (include/mi355x_h264.h, "intra refresh"); it sets slices = n.  Both
    // paths.  Junk, or a conflict with .slices, .refs or .temporallayers (or a picture that has no n bands): one WARN line and the
    // stream the other keys describe
    const std::string refreshKey = GetStrEncParam("persist.vmi.video.encode.intrarefresh");
    bool refreshWarn = false;
    m_intraRefresh = ParseIntraRefresh(refreshKey, cfg.slices, cfg.refs, m_temporalLayers, s.height, &refreshWarn);
    m_lastRefreshBand = -1;
    if (refreshWarn) {
        WARN("intra refresh [%s] rejected (2..32 bands the picture divides into, the same .slices or none, one reference picture, one layer): off",
             refreshKey.c_str());
    }
    if (m_intraRefresh > 0) {
        cfg.slices = m_intraRefresh;
    }
    // extension: "detect" = host pictures go through the damage calls, which transfer only the tiles that changed (include/
    // mi355x_h264.h, "damage tiles"); the bytes of the stream are those of whole pictures.  Stream path and host memory only
    const std::string damageKey = GetStrEncParam("persist.vmi.video.encode.damage");
    const int32_t damage = ParseDamage(damageKey);
    if (damage < 0) {
        WARN("damage [%s] rejected (off | detect): off", damageKey.c_str());
        SetEncParam("persist.vmi.video.encode.damage", "off");
    }
    m_damageDetect = damage > 0;
    m_haveNextDamage = false;
    m_damageInfoSaid = false;
    if (m_damageDetect && (!shared || m_inputDevice)) {
        INFO("damage detect: %s - whole pictures as without the key", !shared ? "an engine of its own has no staging slot to patch (persist.vmi.video.encode.shared = 0)"
                                                                             : "pictures in device memory are read in place, nothing is transferred");
        m_damageDetect = false;
        m_damageInfoSaid = true;
    }
    if (shared) {
        cfg.input_format = m_input;
        uint32_t flags = MI355X_H264_STREAM_MULTIREF;
        if (m_temporalLayers == 2) {
            flags |= MI355X_H264_STREAM_TEMPORAL2;
        }
        if (m_intraRefresh > 0) {
            flags |= MI355X_H264_STREAM_INTRA_REFRESH;
        }
        const int rc = haveColour > 0 ? mi355x_h264_stream_open_colour(&cfg, flags, haveSrc > 0 ? m_srcWidth : cfg.width,
                                                                       haveSrc > 0 ? m_srcHeight : cfg.height, &colour, &m_stream)
                       : haveSrc > 0 ? mi355x_h264_stream_open_scaled(&cfg, flags, m_srcWidth, m_srcHeight, &m_stream)
                                     : mi355x_h264_stream_open_ex(&cfg, flags, &m_stream);
        if (rc != MI355X_H264_OK) {
            ERR("mi355x_h264_stream_open_%s returned %d", haveColour > 0 ? "colour" : haveSrc > 0 ? "scaled" : "ex", rc);
            m_stream = nullptr;
            return false;
        }
        if ((m_psnr || m_ssim) && mi355x_h264_stream_quality_enable_ex(m_stream, metrics) != MI355X_H264_OK) {
            ERR("quality report: %s", mi355x_h264_stream_last_error(m_stream));
            mi355x_h264_stream_close(m_stream);
            m_stream = nullptr;
            return false;
        }
        return true;
    }
    // (an engine of its own takes RGBA through entry points of their own; its input_format names the layout of device I420 / NV12)
    cfg.input_format = m_input == MI355X_H264_INPUT_NV12 ? MI355X_H264_INPUT_NV12 : MI355X_H264_INPUT_I420;
    const int rc = haveColour > 0 ? mi355x_h264_create_colour(&cfg, &colour, &m_engine) : mi355x_h264_create(&cfg, &m_engine);
    if (rc != MI355X_H264_OK) {
        ERR("mi355x_h264_create%s returned %d", haveColour > 0 ? "_colour" : "", rc);
        m_engine = nullptr;
        return false;
    }
    if ((m_psnr || m_ssim) && mi355x_h264_quality_enable_ex(m_engine, metrics) != MI355X_H264_OK) {
        ERR("quality report: %s", mi355x_h264_last_error(m_engine));
        mi355x_h264_destroy(m_engine);
        m_engine = nullptr;
        return false;
    }
    if (m_temporalLayers == 2 && mi355x_h264_set_temporal_layers(m_engine, 2) != MI355X_H264_OK) {
        ERR("temporal layers: %s", mi355x_h264_last_error(m_engine));
        mi355x_h264_destroy(m_engine);
        m_engine = nullptr;
        return false;
    }
    if (m_intraRefresh > 0 && mi355x_h264_set_intra_refresh(m_engine, 1) != MI355X_H264_OK) {
        ERR("intra refresh: %s", mi355x_h264_last_error(m_engine));
        mi355x_h264_destroy(m_engine);
        m_engine = nullptr;
        return false;
    }
    return true;
}

// Quality report of the picture that went out (after a scene-change re-code: the IDR picture's, the last one the engine coded).
// A GOP's line is written when the next IDR picture has been coded, and when the engine closes.
void VideoEncoderMI355X::QualityAfterPicture(bool isIdr)
{
    mi355x_h264_quality q{};
    const int rc = m_stream != nullptr ? mi355x_h264_stream_last_quality(m_stream, &q)
                                       : (mi355x_h264_quality_read(m_engine, &q, 1) == 1 ? MI355X_H264_OK : MI355X_H264_E_ARG);
    m_haveQuality = rc == MI355X_H264_OK;
    m_haveSsim = false;
    if (!m_haveQuality) {
        return;
    }
    m_lastQuality = q;
    if (isIdr) {
        QualityLogGop();
    }
    if (m_ssim) {
        mi355x_h264_ssim s{};
        m_haveSsim = m_stream != nullptr ? mi355x_h264_stream_last_ssim(m_stream, &s) == MI355X_H264_OK
                                         : mi355x_h264_quality_ssim_read(m_engine, &s, 1) == 1;
        if (m_haveSsim) {
            m_lastSsim = s;
            if (s.valid != 0) {
                for (int p = 0; p < 3; p++) {
                    m_gopSsimSum[p] += s.sum[p];
                    m_gopSsimWindows[p] += s.windows[p];
                }
                m_gopSsimPictures++;
            }
        }
    }
    if (q.valid != 0) {
        for (int p = 0; p < 3; p++) {
            m_gopSse[p] += q.sse[p];
            m_gopSamples[p] += q.samples[p];
        }
        m_gopBytes += q.bytes;
        m_gopPictures++;
    }
}

// pictures, mean bytes and mean PSNR Y / U / V of the GOP that has ended: the PSNR of the GOP's mean squared error per plane
// (10 log10(255^2 samples / SSE) over the sums; computed here, on the host - the library reports integers only)
void VideoEncoderMI355X::QualityLogGop()
{
    if (m_gopPictures != 0 && m_psnr) {
        double db[3];
        for (int p = 0; p < 3; p++) {
            db[p] = m_gopSse[p] != 0 ? 10.0 * std::log10(65025.0 * static_cast<double>(m_gopSamples[p]) / static_cast<double>(m_gopSse[p])) : INFINITY;
        }
        INFO("GOP of %u pictures: mean %llu bytes, mean PSNR Y %.2f U %.2f V %.2f dB", m_gopPictures,
             static_cast<unsigned long long>(m_gopBytes / m_gopPictures), db[0], db[1], db[2]);
    }
    for (int p = 0; p < 3; p++) {
        m_gopSse[p] = m_gopSamples[p] = 0;
    }
    m_gopBytes = 0;
    m_gopPictures = 0;
    // a line of its own: the mean SSIM Y / U / V of the GOP, sum / (65536 windows) over the GOP's sums (computed here, on the host)
    if (m_gopSsimPictures != 0) {
        double mean[3];
        for (int p = 0; p < 3; p++) {
            mean[p] = m_gopSsimWindows[p] != 0 ? static_cast<double>(m_gopSsimSum[p]) / (65536.0 * static_cast<double>(m_gopSsimWindows[p])) : NAN;
        }
        INFO("GOP of %u pictures: mean SSIM Y %.4f U %.4f V %.4f", m_gopSsimPictures, mean[0], mean[1], mean[2]);
    }
    for (int p = 0; p < 3; p++) {
        m_gopSsimSum[p] = 0;
        m_gopSsimWindows[p] = 0;
    }
    m_gopSsimPictures = 0;
}

bool VideoEncoderMI355X::LastFrameQuality(mi355x_h264_quality *out) const
{
    if ((!m_psnr && !m_ssim) || !m_haveQuality || out == nullptr) {
        return false;
    }
    *out = m_lastQuality;
    return true;
}

bool VideoEncoderMI355X::LastFrameSsim(mi355x_h264_ssim *out) const
{
    if (!m_ssim || !m_haveSsim || out == nullptr) {
        return false;
    }
    *out = m_lastSsim;
    return true;
}

// Frame-level rate control for the bitrate mode: GOP budget + damped QP steps, the C++ statement of media_amd/ratecontrol.py
// (integer for integer; a test replays the QP sequence on the oracle).  A GOP has target * gop bits, less the debt the virtual
// buffer carries into it (within [1/2, 3/2] of that); the IDR picture is paid out of it and every P picture is budgeted (what is
// left) / (pictures left).  The QP moves by one step when the running mean of the P pictures' bits (3/4 old + 1/4 new) is 15 %
// over or 13 % under the next picture's budget, by two beyond 3/2 and 2/3.
// PARITY UNPINNED: OpenH264's own rate-control model is not available.
void VideoEncoderMI355X::RateControlUpdate(uint32_t frameBytes, bool isIdr)
{
    if (m_fixedQp >= 0) {
        return;
    }
    const int64_t rate = static_cast<int64_t>(Active().bitrate);
    const int64_t target = rate / std::max<uint32_t>(1, Active().fps);
    const int64_t gop = std::max<int64_t>(1, static_cast<int64_t>(Active().gop));
    const int64_t bits = static_cast<int64_t>(frameBytes) * 8;
    const int64_t debt = m_bufferBits;
    m_bufferBits = std::max<int64_t>(m_bufferBits + bits - target, -rate);
    int64_t est;
    if (isIdr || m_picsLeft <= 0) {
        const int64_t full = target * gop;
        const int64_t budget = std::min(std::max(full - debt, full / 2), full * 3 / 2);
        m_gopLeft = budget - bits;
        m_picsLeft = gop - 1;
        est = m_meanP != 0 ? m_meanP : bits / 9;   // (no P picture yet: an IDR picture costs about nine of them)
    } else {
        m_gopLeft -= bits;
        m_picsLeft -= 1;
        m_meanP = m_meanP != 0 ? (m_meanP * 3 + bits) / 4 : bits;
        est = m_meanP;
    }
    // (floor division as in the Python statement: m_gopLeft may be negative)
    const int64_t n = std::max<int64_t>(1, m_picsLeft);
    int64_t share = m_gopLeft / n;
    if (m_gopLeft < 0 && m_gopLeft % n != 0) {
        share -= 1;
    }
    const int64_t next = std::max(share, target / 4);
    int32_t step = 0;
    if (est * 2 > next * 3) {
        step = 2;
    } else if (est * 100 > next * 115) {
        step = 1;
    } else if (est * 3 < next * 2) {
        step = -2;
    } else if (est * 100 < next * 87) {
        step = -1;
    }
    m_qp = std::min(Rc::kQpMax, std::max(Rc::kQpMin, m_qp + step));
}

// QP of a stream's first picture from its bits per pixel (media_amd/ratecontrol.py start_qp)
int32_t VideoEncoderMI355X::StartQp(uint32_t bitrate, uint32_t fps, uint32_t width, uint32_t height)
{
    const int64_t mbpp = static_cast<int64_t>(bitrate) * 1000 / std::max<int64_t>(1, static_cast<int64_t>(fps) * width * height);
    static const struct { int64_t lim; int32_t qp; } table[] = {{200, 24}, {100, 27}, {50, 30}, {25, 34}, {12, 38}};
    for (const auto &t : table) {
        if (mbpp >= t.lim) {
            return t.qp;
        }
    }
    return 42;
}

int32_t VideoEncoderMI355X::ParseInputLayout(const std::string &value)
{
    return value == "nv12" ? MI355X_H264_INPUT_NV12 : value == "rgba" ? MI355X_H264_INPUT_RGBA : MI355X_H264_INPUT_I420;
}

int32_t VideoEncoderMI355X::ParseRefs(const std::string &value) { return value == "2" ? 2 : value == "3" ? 3 : 1; }

bool VideoEncoderMI355X::ParsePsnr(const std::string &value) { return value == "1"; }

int32_t VideoEncoderMI355X::ParseTemporalLayers(const std::string &value, bool *junk)
{
    if (junk != nullptr) {
        *junk = !(value.empty() || value == "1" || value == "2");
    }
    return value == "2" ? 2 : 1;
}

int32_t VideoEncoderMI355X::ParseIntraRefresh(const std::string &value, int32_t slices, int32_t refs, int32_t layers, uint32_t height, bool *warn)
{
    if (warn != nullptr) {
        *warn = false;
    }
    if (value.empty()) {
        return 0;
    }
    int32_t n = 0;
    bool ok = value.size() <= 2 && value[0] != '0';
    for (char ch : value) {
        ok = ok && ch >= '0' && ch <= '9';
        n = n * 10 + (ch - '0');
    }
    ok = ok && n >= 2 && n <= 32;
    if (ok) {   // the bands the engine makes of n slices: ceil(rows / n) macroblock rows each, two at least
        const int32_t mbh = (static_cast<int32_t>(height) + 15) / 16;
        const int32_t m = std::min(n, std::max(1, mbh / 2)), rows = (mbh + m - 1) / m;
        ok = (mbh + rows - 1) / rows == n;
    }
    ok = ok && (slices == 0 || slices == n) && refs <= 1 && layers == 1;
    if (!ok && warn != nullptr) {
        *warn = true;
    }
    return ok ? n : 0;
}

bool VideoEncoderMI355X::ParseSsim(const std::string &value) { return value == "1"; }

int32_t VideoEncoderMI355X::ParseDamage(const std::string &value) { return damage::parse_mode_key(value.c_str()); }

bool VideoEncoderMI355X::SetNextDamage(const Rect *rects, int n)
{
    if (n < 0 || (n > 0 && rects == nullptr)) {
        return false;
    }
    for (int i = 0; i < n; i++) {
        if (rects[i].w < 0 || rects[i].h < 0) {
            return false;
        }
    }
    m_nextDamage.assign(rects, rects + n);
    m_haveNextDamage = true;
    return true;
}

bool VideoEncoderMI355X::LastUpload(uint64_t *bytes, uint32_t *tiles, uint32_t *tilesTotal, int *mode) const
{
    return m_stream != nullptr && mi355x_h264_stream_last_upload(m_stream, bytes, tiles, tilesTotal, mode) == MI355X_H264_OK;
}

int VideoEncoderMI355X::ParseColour(const std::string &colour, const std::string &range, mi355x_h264_colour *out)
{
    if (colour.empty() && range.empty()) {
        return 0;
    }
    const bool colourOk = colour.empty() || colour == "bt601" || colour == "bt709";
    const bool rangeOk = range.empty() || range == "limited" || range == "full";
    if (!colourOk || !rangeOk) {
        return -1;
    }
    out->struct_size = sizeof(*out);
    out->matrix = colour == "bt709" ? MI355X_H264_MATRIX_BT709 : MI355X_H264_MATRIX_BT601;
    out->full_range = range == "full" ? 1 : 0;
    return 1;
}

bool VideoEncoderMI355X::Colour(mi355x_h264_colour *out) const
{
    if (m_stream != nullptr) {
        return mi355x_h264_stream_colour(m_stream, out) == 1;
    }
    return m_engine != nullptr && mi355x_h264_colour_of(m_engine, out) == 1;
}

bool VideoEncoderMI355X::ParseInputDevice(const std::string &value) { return value == "device"; }

int VideoEncoderMI355X::ParseSourceSize(const std::string &width, const std::string &height, uint32_t codedWidth, uint32_t codedHeight,
                                        int32_t *srcWidth, int32_t *srcHeight)
{
    if (width.empty() && height.empty()) {
        return 0;
    }
    auto number = [](const std::string &v) {   // 1 .. 5 decimal digits and nothing else; -1 otherwise
        if (v.empty() || v.size() > 5 || v.find_first_not_of("0123456789") != std::string::npos) {
            return -1;
        }
        return atoi(v.c_str());
    };
    const int32_t w = number(width), h = number(height);
    const int64_t cw = codedWidth, ch = codedHeight;
    if (((w | h) & 1) != 0 || !Within(w, 16, 4096) || !Within(h, 16, 4096) || w < cw || h < ch || w > 4 * cw || h > 4 * ch) {
        return -1;
    }
    *srcWidth = w;
    *srcHeight = h;
    return 1;
}

int VideoEncoderMI355X::EncodePicture(const uint8_t *i420, uint8_t **out, uint32_t *outLen, int *frameType)
{
    if (m_inputDevice) {   // one tight picture in device memory, in the object's layout
        if (m_haveNextDamage && !m_damageInfoSaid) {
            INFO("SetNextDamage: pictures in device memory are read in place, nothing is transferred");
            m_damageInfoSaid = true;
        }
        if (m_stream != nullptr) {
            return mi355x_h264_stream_encode_device(m_stream, i420, out, outLen, frameType);
        }
        return m_input == MI355X_H264_INPUT_RGBA ? mi355x_h264_encode_rgba_device(m_engine, i420, out, outLen, frameType)
                                                 : mi355x_h264_encode_device(m_engine, i420, out, outLen, frameType);
    }
    // damage tiles: the rectangles of SetNextDamage, else what the key says; stream path only (EngineOpen has said so for the key)
    const bool useDamage = m_stream != nullptr && (m_haveNextDamage || m_damageDetect);
    if (m_haveNextDamage && m_stream == nullptr && !m_damageInfoSaid) {
        INFO("SetNextDamage: an engine of its own has no staging slot to patch - whole pictures");
        m_damageInfoSaid = true;
    }
    const mi355x_h264_rect *rects = m_haveNextDamage && !m_nextDamage.empty() ? m_nextDamage.data() : nullptr;
    const int nrects = m_haveNextDamage ? static_cast<int>(m_nextDamage.size()) : MI355X_H264_DAMAGE_DETECT;
    if (useDamage && m_input == MI355X_H264_INPUT_RGBA) {
        return mi355x_h264_stream_encode_rgba_damage(m_stream, i420, static_cast<int>(SrcWidth()) * 4, rects, nrects, out, outLen, frameType);
    }
    if (useDamage && m_input == MI355X_H264_INPUT_NV12) {
        const int w = static_cast<int>(SrcWidth());
        return mi355x_h264_stream_encode_nv12_damage(m_stream, i420, w, i420 + SrcLumaBytes(), w, rects, nrects, out, outLen, frameType);
    }
    if (useDamage) {
        const int pitch = static_cast<int>(SrcWidth());
        const uint8_t *u = i420 + SrcLumaBytes();
        return mi355x_h264_stream_encode_damage(m_stream, i420, pitch, u, pitch / 2, u + SrcLumaBytes() / 4, pitch / 2, rects, nrects, out, outLen, frameType);
    }
    if (m_input == MI355X_H264_INPUT_RGBA) {
        const int stride = static_cast<int>(SrcWidth()) * 4;
        return m_stream != nullptr ? mi355x_h264_stream_encode_rgba(m_stream, i420, stride, out, outLen, frameType)
                                   : mi355x_h264_encode_rgba(m_engine, i420, stride, out, outLen, frameType);
    }
    if (m_input == MI355X_H264_INPUT_NV12) {
        const int w = static_cast<int>(SrcWidth());
        return m_stream != nullptr ? mi355x_h264_stream_encode_nv12(m_stream, i420, w, i420 + SrcLumaBytes(), w, out, outLen, frameType)
                                   : mi355x_h264_encode_nv12(m_engine, i420, w, i420 + SrcLumaBytes(), w, out, outLen, frameType);
    }
    // tight I420 exactly as the reference's InitSrcPic lays the planes out (ref :354-365)
    const int pitch = static_cast<int>(SrcWidth());
    const uint8_t *u = i420 + SrcLumaBytes();
    const uint8_t *v = u + SrcLumaBytes() / 4;
    if (m_stream != nullptr) {
        return mi355x_h264_stream_encode(m_stream, i420, pitch, u, pitch / 2, v, pitch / 2, out, outLen, frameType);
    }
    return mi355x_h264_encode(m_engine, i420, pitch, u, pitch / 2, v, pitch / 2, out, outLen, frameType);
}

bool VideoEncoderMI355X::EngineEncode(const uint8_t *i420, uint8_t **out, uint32_t *outLen)
{
    if (m_stream != nullptr) {
        (void) mi355x_h264_stream_set_qp(m_stream, m_qp);
    } else {
        (void) mi355x_h264_set_qp(m_engine, m_qp);
    }
    m_lastQp = m_qp;
    int frameType = 0;
    int rc = EncodePicture(i420, out, outLen, &frameType);
    if (rc == MI355X_H264_OK && m_sceneDetect && frameType == MI355X_H264_FRAME_P) {
        // scene change: the motion search found no good match anywhere -> code this picture as IDR instead
        uint32_t cost = 0;
        const uint64_t mbs = static_cast<uint64_t>((Active().width + 15) / 16) * ((Active().height + 15) / 16);
        const int crc = m_stream != nullptr ? mi355x_h264_stream_last_me_cost(m_stream, &cost) : mi355x_h264_last_me_cost(m_engine, &cost);
        if (crc == MI355X_H264_OK && cost > Rc::kSceneCutCostPerMb * mbs) {
            INFO("scene change (motion cost %u over %llu macroblocks): picture re-coded as IDR", cost,
                 static_cast<unsigned long long>(mbs));
            (void) EngineForceIdr();
            rc = EncodePicture(i420, out, outLen, &frameType);
            m_sceneCuts++;
        }
    }
    m_haveNextDamage = false;   // (SetNextDamage holds for this picture alone, its re-code included)
    if (rc != MI355X_H264_OK) {
        ERR("EncodeOneFrame: engine returned %d (%s)", rc,
            m_stream != nullptr ? mi355x_h264_stream_last_error(m_stream) : mi355x_h264_last_error(m_engine));
        return false;
    }
    m_lastTemporalId = m_stream != nullptr ? mi355x_h264_stream_last_temporal_id(m_stream) : mi355x_h264_last_temporal_id(m_engine);
    m_lastRefreshBand = m_stream != nullptr ? mi355x_h264_stream_last_refresh_band(m_stream) : mi355x_h264_last_refresh_band(m_engine);
    if (m_psnr || m_ssim) {
        QualityAfterPicture(frameType == MI355X_H264_FRAME_IDR);
    }
    RateControlUpdate(*outLen, frameType == MI355X_H264_FRAME_IDR);
    return true;
}

void VideoEncoderMI355X::EngineClose()
{
    if ((m_psnr || m_ssim) && (m_engine != nullptr || m_stream != nullptr)) {
        QualityLogGop();
    }
    if (m_engine != nullptr) {
        mi355x_h264_destroy(m_engine);
        m_engine = nullptr;
    }
    if (m_stream != nullptr) {
        mi355x_h264_stream_close(m_stream);
        m_stream = nullptr;
    }
}

bool VideoEncoderMI355X::EngineForceIdr()
{
    if (m_stream != nullptr) {
        return mi355x_h264_stream_force_idr(m_stream) == MI355X_H264_OK;
    }
    return m_engine != nullptr && mi355x_h264_force_idr(m_engine) == MI355X_H264_OK;
}

int64_t VideoEncoderMI355X::ReadReconY(void *dst, size_t cap, int32_t *codedWidth, int32_t *codedHeight)
{
    if (m_stream != nullptr) {
        if (codedWidth != nullptr) *codedWidth = mi355x_h264_stream_coded_width(m_stream);
        if (codedHeight != nullptr) *codedHeight = mi355x_h264_stream_coded_height(m_stream);
        return mi355x_h264_stream_debug_read(m_stream, MI355X_H264_DBG_RECON_Y, dst, cap);
    }
    if (m_engine == nullptr) return -1;
    if (codedWidth != nullptr) *codedWidth = mi355x_h264_coded_width(m_engine);
    if (codedHeight != nullptr) *codedHeight = mi355x_h264_coded_height(m_engine);
    return mi355x_h264_debug_read(m_engine, MI355X_H264_DBG_RECON_Y, dst, cap);
}
