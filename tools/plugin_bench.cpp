// tools/plugin_bench.cpp -- native measurement of the drop-in boundary in the reference's operating mode: S host threads, each
// CreateVideoEncoder -> InitEncoder -> StartEncoder -> EncodeOneFrame x F on host I420 pictures (bitrate mode, scene detection
// on), compiled against include/VideoCodecApi.h and linked with libVideoCodec.so.  No Python in the timed region (bench.py's
// own plugin harness holds the interpreter lock between calls); bench.py --mode plugin runs this binary when it has been built
// (media_amd/lib/plugin_bench, recipe in media_amd/host/Makefile).  Configuration reaches the library through the property
// store, seeded from environment variables as in tests/boundary/ref_header_caller.cpp.
//
// usage: plugin_bench [--damage detect] [--static-share P] [--intra-refresh N] [--temporal N] [--refs N] [--psnr] [--ssim] [--src WxH] [--colour bt601|bt709] [--range limited|full] <i420 file with N pictures> <width> <height> <N> <frames per stream> <S1,S2,...> [input]
// prints one JSON object per S on its own line.
// --damage detect (anywhere on the line): the extension key persist.vmi.video.encode.damage = detect - every host picture goes through
// the damage call, which transfers only the tiles that changed (include/mi355x_h264.h, "damage tiles").  With or without it the JSON
// line carries upload_bytes_per_picture, link_gbps and damaged_tiles_per_picture / tiles_total from every picture's
// mi355x_h264_stream_last_upload (read after its call, outside the latency sample).
// --static-share P (anywhere on the line; host pictures only): content option - every stream keeps a picture of its own, and each
// picture differs from the stream's last one only inside a window of consecutive tiles (64 x 16, raster order, wrapping) that covers
// 100 - P % of the grid and moves by half its length per picture; inside the window the bytes come from the next picture of the
// file, the rest is byte-identical.  The window is copied before the call's clock starts but inside the run's, with and without
// --damage alike.
// --refs N (anywhere on the line): the extension key persist.vmi.video.encode.refs = N - 2 or 3 reference pictures are searched
// (every object a stream of a shared engine that keeps N + 1 reconstructions per stream); without it the key is left as found.
// --temporal N (anywhere on the line): the extension key persist.vmi.video.encode.temporallayers = N - with 2 every second P picture
// of a GOP is a non-reference picture (include/mi355x_h264.h, "temporal layers"); every picture's layer is read after its call
// (outside the latency sample), and the JSON line carries pictures_l0 / pictures_l1 and bytes_l0 / bytes_l1.
// --intra-refresh N (anywhere on the line): the extension key persist.vmi.video.encode.intrarefresh = N - N slice bands, one of them
// all intra in every P picture (include/mi355x_h264.h, "intra refresh").  Compare with a run that sets
// PERSIST_VMI_VIDEO_ENCODE_SLICES=N instead: the same slices without the refresh.
// --ssim (anywhere on the line): the extension key persist.vmi.video.encode.ssim = 1 - the report is on with both metrics, every
// picture's SSIM record is read after its call (outside the latency sample), and the JSON line carries ssim_y / ssim_u / ssim_v:
// sum / (65536 windows) over all pictures of the run, per plane.
// --psnr (anywhere on the line): the extension key persist.vmi.video.encode.psnr = 1 - the library's quality report is on, every
// picture's record is read after its call (outside the latency sample), and the JSON line carries psnr_y / psnr_u / psnr_v: the
// PSNR of the mean squared error of all pictures of the run, per plane.
// --src WxH (anywhere on the line): the extension keys persist.vmi.video.encode.srcwidth / .srcheight = W / H - the file holds
// pictures of W x H, which every object hands over as they are and the device resamples to the coded size (<width> <height> and
// the geometry keys stay the coded size's).
// --colour C / --range R (anywhere on the line): the extension keys persist.vmi.video.encode.colour / .range - every object's
// stream carries that colour description in its SPS, and RGBA pictures are converted with it (include/mi355x_h264.h, "colour
// description"); the values go to the library as they are, which takes bt601 | bt709 and limited | full.
// input (optional; without it everything is as above): i420 | nv12 | rgba, with ":device" behind it for pictures in device
// memory - the extension keys persist.vmi.video.encode.input / .inputmem.  The pictures of the file are converted to the layout
// on the host before the clock starts; for device memory they are uploaded once, before the clock, and every stream cycles
// through them in place (the HIP runtime is reached through dlopen: this tool is built with the host compiler alone).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <thread>
#include <vector>
#include <cmath>
#include "VideoCodecApi.h"
#include "mi355x_h264.h"
#include "../media_amd/csrc/damage.h"   // the tile grid (plain C++)

extern "C" int32_t vc_last_quality(void *enc, mi355x_h264_quality *out);   // media_amd/host/capi_shim.cpp
extern "C" int32_t vc_last_ssim(void *enc, mi355x_h264_ssim *out);
extern "C" int32_t vc_last_temporal_id(void *enc);
extern "C" int32_t vc_last_upload(void *enc, uint64_t *bytes, uint32_t *tiles, uint32_t *tilesTotal, int32_t *mode);

int main(int argc, char **argv)
{
    for (int i = 1; i + 1 < argc; i++)   // --refs N: taken out of the line, the rest is positional
        if (strcmp(argv[i], "--refs") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_REFS", argv[i + 1], 1);
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; i++)   // --damage detect: taken out of the line
        if (strcmp(argv[i], "--damage") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_DAMAGE", argv[i + 1], 1);
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    int staticShare = -1;
    for (int i = 1; i + 1 < argc; i++)   // --static-share P: taken out of the line
        if (strcmp(argv[i], "--static-share") == 0) {
            staticShare = atoi(argv[i + 1]);
            if (staticShare < 0 || staticShare > 100) { fprintf(stderr, "--static-share %s: 0 .. 100 expected\n", argv[i + 1]); return 2; }
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool temporal = false;
    for (int i = 1; i + 1 < argc; i++)   // --temporal N: taken out of the line
        if (strcmp(argv[i], "--temporal") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_TEMPORALLAYERS", argv[i + 1], 1);
            temporal = true;
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (int i = 1; i + 1 < argc; i++)   // --intra-refresh N: taken out of the line
        if (strcmp(argv[i], "--intra-refresh") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_INTRAREFRESH", argv[i + 1], 1);
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    bool psnr = false;
    for (int i = 1; i < argc; i++)   // --psnr: taken out of the line
        if (strcmp(argv[i], "--psnr") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_PSNR", "1", 1);
            psnr = true;
            for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    int srcW = 0, srcH = 0;
    for (int i = 1; i + 1 < argc; i++)   // --src WxH: taken out of the line
        if (strcmp(argv[i], "--src") == 0) {
            if (sscanf(argv[i + 1], "%dx%d", &srcW, &srcH) != 2 || srcW < 16 || srcH < 16) { fprintf(stderr, "--src %s: WxH expected\n", argv[i + 1]); return 2; }
            setenv("PERSIST_VMI_VIDEO_ENCODE_SRCWIDTH", std::to_string(srcW).c_str(), 1);
            setenv("PERSIST_VMI_VIDEO_ENCODE_SRCHEIGHT", std::to_string(srcH).c_str(), 1);
            for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    for (const char *opt : {"--colour", "--range"})   // --colour C, --range R: taken out of the line
        for (int i = 1; i + 1 < argc; i++)
            if (strcmp(argv[i], opt) == 0) {
                setenv(strcmp(opt, "--colour") == 0 ? "PERSIST_VMI_VIDEO_ENCODE_COLOUR" : "PERSIST_VMI_VIDEO_ENCODE_RANGE", argv[i + 1], 1);
                for (int j = i; j + 2 < argc; j++) argv[j] = argv[j + 2];
                argc -= 2;
                break;
            }
    bool ssim = false;
    for (int i = 1; i < argc; i++)   // --ssim: taken out of the line
        if (strcmp(argv[i], "--ssim") == 0) {
            setenv("PERSIST_VMI_VIDEO_ENCODE_SSIM", "1", 1);
            ssim = true;
            for (int j = i; j + 1 < argc; j++) argv[j] = argv[j + 1];
            argc -= 1;
            break;
        }
    if (argc != 7 && argc != 8) { fprintf(stderr, "usage: %s [--damage detect] [--static-share P] [--intra-refresh N] [--temporal N] [--refs N] [--psnr] [--ssim] [--src WxH] [--colour bt601|bt709] [--range limited|full] in.i420 w h pictures frames_per_stream S1,S2,... [i420|nv12|rgba[:device]]\n", argv[0]); return 2; }
    // (w, h: the size of the pictures in the file and in every call - the source size with --src)
    const int w = srcW > 0 ? srcW : atoi(argv[2]), h = srcW > 0 ? srcH : atoi(argv[3]), npic = atoi(argv[4]), frames = atoi(argv[5]);
    size_t fsz = (size_t)w * h * 3 / 2;
    std::vector<uint8_t> pics(fsz * npic);
    FILE *in = fopen(argv[1], "rb");
    if (in == nullptr || fread(pics.data(), 1, pics.size(), in) != pics.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(in);
    const uint8_t *base = pics.data();   // where the pictures lie: fsz bytes apart, in host or in device memory
    std::string layout = argc == 8 ? argv[7] : "i420";
    bool device = false;
    if (layout.size() > 7 && layout.compare(layout.size() - 7, 7, ":device") == 0) { device = true; layout.resize(layout.size() - 7); }
    if (layout != "i420" && layout != "nv12" && layout != "rgba") { fprintf(stderr, "unknown input %s\n", argv[7]); return 2; }
    if (argc == 8) {
        setenv("PERSIST_VMI_VIDEO_ENCODE_INPUT", layout.c_str(), 1);
        setenv("PERSIST_VMI_VIDEO_ENCODE_INPUTMEM", device ? "device" : "", 1);
    }
    if (layout != "i420") {   // the same pictures in the other layout (RGBA: BT.601 back to RGB, any mapping will do for a measurement)
        const size_t ysz = (size_t)w * h, nsz = layout == "rgba" ? ysz * 4 : fsz;
        std::vector<uint8_t> conv(nsz * npic);
        for (int p = 0; p < npic; p++) {
            const uint8_t *Y = pics.data() + fsz * p, *U = Y + ysz, *V = U + ysz / 4;
            uint8_t *o = conv.data() + nsz * p;
            if (layout == "nv12") {
                memcpy(o, Y, ysz);
                for (size_t i = 0; i < ysz / 4; i++) { o[ysz + 2 * i] = U[i]; o[ysz + 2 * i + 1] = V[i]; }
            } else {
                auto clip = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++) {
                        const int l = Y[(size_t)y * w + x], cb = U[(size_t)(y / 2) * (w / 2) + x / 2] - 128, cr = V[(size_t)(y / 2) * (w / 2) + x / 2] - 128;
                        uint8_t *q = o + ((size_t)y * w + x) * 4;
                        q[0] = clip(l + ((359 * cr) >> 8)); q[1] = clip(l - ((88 * cb + 183 * cr) >> 8)); q[2] = clip(l + ((454 * cb) >> 8)); q[3] = 255;
                    }
            }
        }
        pics.swap(conv);
        fsz = nsz;
        base = pics.data();
    }
    if (device && staticShare >= 0) { fprintf(stderr, "--static-share makes host pictures\n"); return 2; }
    const int dlayout = layout == "rgba" ? damage::LAYOUT_RGBA : layout == "nv12" ? damage::LAYOUT_NV12 : damage::LAYOUT_I420;
    const int ntiles = damage::tiles_total(w, h), nwin = staticShare < 0 ? 0 : (int)(((int64_t)ntiles * (100 - staticShare) + 50) / 100);
    if (device) {   // upload once, before the clock
        void *hip = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
        auto dmalloc = hip ? reinterpret_cast<int (*)(void **, size_t)>(dlsym(hip, "hipMalloc")) : nullptr;
        auto dcopy = hip ? reinterpret_cast<int (*)(void *, const void *, size_t, int)>(dlsym(hip, "hipMemcpy")) : nullptr;
        void *d = nullptr;
        if (!dmalloc || !dcopy || dmalloc(&d, pics.size()) != 0 || dcopy(d, pics.data(), pics.size(), 1 /* hipMemcpyHostToDevice */) != 0) {
            fprintf(stderr, "cannot put the pictures into device memory\n");
            return 2;
        }
        base = static_cast<const uint8_t *>(d);
    }
    std::vector<int> counts;
    for (char *tok = strtok(argv[6], ","); tok != nullptr; tok = strtok(nullptr, ",")) counts.push_back(atoi(tok));
    for (int S : counts) {
        std::vector<VideoEncoder *> encs(S, nullptr);
        bool ok = true;
        for (int k = 0; k < S && ok; k++) {
            ok = CreateVideoEncoder(&encs[k]) == VIDEO_ENCODER_SUCCESS && encs[k] != nullptr && encs[k]->InitEncoder() == VIDEO_ENCODER_SUCCESS &&
                 encs[k]->StartEncoder() == VIDEO_ENCODER_SUCCESS;
            if (ok) {   // warm-up outside the clock: first IDR, allocations
                uint8_t *au = nullptr;
                uint32_t n = 0;
                ok = encs[k]->EncodeOneFrame(base + fsz * (size_t)(k % npic), (uint32_t)fsz, &au, &n) == VIDEO_ENCODER_SUCCESS;
            }
        }
        if (!ok) { printf("{\"streams\":%d,\"error\":\"an encoder could not be opened\"}\n", S); continue; }
        std::vector<std::vector<double>> lat(S);
        std::vector<uint64_t> bytes(S, 0);
        std::atomic<int> failures{0};
        std::vector<uint64_t> sse((size_t)S * 3, 0), samples((size_t)S * 3, 0), windows((size_t)S * 3, 0);
        std::vector<int64_t> qsum((size_t)S * 3, 0);
        std::vector<uint64_t> lpics((size_t)S * 2, 0), lbytes((size_t)S * 2, 0);   // per temporal layer
        std::vector<uint64_t> upBytes(S, 0), upTiles(S, 0);
        // --static-share: every stream's own picture, as the warm-up call left it in the library
        std::vector<std::vector<uint8_t>> own(staticShare >= 0 ? S : 0);
        for (int k = 0; k < (int)own.size(); k++) own[k].assign(base + fsz * (size_t)(k % npic), base + fsz * (size_t)(k % npic) + fsz);
        auto work = [&](int k) {
            lat[k].reserve(frames);
            std::vector<uint8_t> mark;
            for (int i = 0; i < frames; i++) {
                const uint8_t *f = base + fsz * (size_t)((k + 1 + i) % npic);   // (the pool holds frames + S + 1 pictures: no wrap)
                if (staticShare >= 0) {   // the window's tiles from the pool's picture into the stream's own
                    mark.assign((size_t)ntiles, 0);
                    const int start = nwin ? (int)(((int64_t)i * (nwin / 2 + 1) + 7 * k) % ntiles) : 0;
                    for (int t = 0; t < nwin; t++) mark[(size_t)((start + t) % ntiles)] = 1;
                    const size_t ysz = (size_t)w * h;
                    const damage::Picture src{dlayout, {f, f + ysz, f + ysz + ysz / 4}, {dlayout == damage::LAYOUT_RGBA ? 4 * w : w, dlayout == damage::LAYOUT_I420 ? w / 2 : w, w / 2}};
                    damage::copy_tiles(src, w, h, mark, own[k].data());
                    f = own[k].data();
                }
                uint8_t *au = nullptr;
                uint32_t n = 0;
                const auto t0 = std::chrono::steady_clock::now();
                const EncoderRetCode rc = encs[k]->EncodeOneFrame(f, (uint32_t)fsz, &au, &n);
                lat[k].push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                if (rc != VIDEO_ENCODER_SUCCESS) failures++;
                else bytes[k] += n;
                uint64_t ub = 0; uint32_t ut = 0, utt = 0; int32_t um = 0;
                if (rc == VIDEO_ENCODER_SUCCESS && vc_last_upload(encs[k], &ub, &ut, &utt, &um) == 0) { upBytes[k] += ub; upTiles[k] += ut; }
                if (temporal && rc == VIDEO_ENCODER_SUCCESS) {
                    const int tid = vc_last_temporal_id(encs[k]) == 1 ? 1 : 0;
                    lpics[(size_t)k * 2 + tid]++; lbytes[(size_t)k * 2 + tid] += n;
                }
                mi355x_h264_quality q;
                if (psnr && rc == VIDEO_ENCODER_SUCCESS && vc_last_quality(encs[k], &q) == 0 && q.valid)
                    for (int p = 0; p < 3; p++) { sse[(size_t)k * 3 + p] += q.sse[p]; samples[(size_t)k * 3 + p] += q.samples[p]; }
                mi355x_h264_ssim sq;
                if (ssim && rc == VIDEO_ENCODER_SUCCESS && vc_last_ssim(encs[k], &sq) == 0 && sq.valid)
                    for (int p = 0; p < 3; p++) { qsum[(size_t)k * 3 + p] += sq.sum[p]; windows[(size_t)k * 3 + p] += sq.windows[p]; }
            }
        };
        std::vector<std::thread> ths;
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < S; k++) ths.emplace_back(work, k);
        for (auto &t : ths) t.join();
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (auto *e : encs) { e->StopEncoder(); e->DestroyEncoder(); DestroyVideoEncoder(e); }
        std::vector<double> all;
        uint64_t total = 0;
        for (int k = 0; k < S; k++) { all.insert(all.end(), lat[k].begin(), lat[k].end()); total += bytes[k]; }
        std::sort(all.begin(), all.end());
        const size_t n = all.size();
        char q[720] = "";
        {
            uint64_t ub = 0, ut = 0;
            for (int k = 0; k < S; k++) { ub += upBytes[k]; ut += upTiles[k]; }
            snprintf(q, sizeof(q), ",\"upload_bytes_per_picture\":%.1f,\"link_gbps\":%.3f,\"damaged_tiles_per_picture\":%.1f,\"tiles_total\":%d,\"static_share\":%d",
                     (double)ub / n, (double)ub / dt / 1e9, (double)ut / n, ntiles, staticShare);
        }
        if (temporal) {
            uint64_t np[2] = {0, 0}, nb[2] = {0, 0};
            for (int k = 0; k < S; k++)
                for (int l = 0; l < 2; l++) { np[l] += lpics[(size_t)k * 2 + l]; nb[l] += lbytes[(size_t)k * 2 + l]; }
            const size_t at = strlen(q);
            snprintf(q + at, sizeof(q) - at, ",\"pictures_l0\":%llu,\"pictures_l1\":%llu,\"bytes_l0\":%llu,\"bytes_l1\":%llu", (unsigned long long)np[0],
                     (unsigned long long)np[1], (unsigned long long)nb[0], (unsigned long long)nb[1]);
        }
        if (psnr) {
            double db[3];
            for (int p = 0; p < 3; p++) {
                uint64_t e = 0, m = 0;
                for (int k = 0; k < S; k++) { e += sse[(size_t)k * 3 + p]; m += samples[(size_t)k * 3 + p]; }
                db[p] = m == 0 ? 0.0 : (e == 0 ? 999.0 : 10.0 * std::log10(65025.0 * (double)m / (double)e));   // (999: no error at all)
            }
            const size_t at = strlen(q);
            snprintf(q + at, sizeof(q) - at, ",\"psnr_y\":%.3f,\"psnr_u\":%.3f,\"psnr_v\":%.3f", db[0], db[1], db[2]);
        }
        if (ssim) {
            double mean[3];
            for (int p = 0; p < 3; p++) {
                int64_t t = 0; uint64_t m = 0;
                for (int k = 0; k < S; k++) { t += qsum[(size_t)k * 3 + p]; m += windows[(size_t)k * 3 + p]; }
                mean[p] = m == 0 ? 0.0 : (double)t / (65536.0 * (double)m);
            }
            const size_t at = strlen(q);
            snprintf(q + at, sizeof(q) - at, ",\"ssim_y\":%.5f,\"ssim_u\":%.5f,\"ssim_v\":%.5f", mean[0], mean[1], mean[2]);
        }
        printf("{\"streams\":%d,\"fps_aggregate\":%.1f,\"fps_per_stream\":%.1f,\"latency_ms_p50\":%.3f,\"latency_ms_p99\":%.3f,\"bytes_per_picture\":%.1f,"
               "\"bitrate_achieved\":%.0f,\"pictures\":%zu,\"encode_failures\":%d%s}\n",
               S, n / dt, n / dt / S, all[n / 2], all[std::min(n - 1, (size_t)(n * 0.99))], (double)total / n, (double)total * 8 * 30 / n, n, failures.load(), q);
        fflush(stdout);
    }
    return 0;
}
