// tools/ubench_scale.hip -- the scaling ingest alone (media_amd/csrc/scale_kernels.h, launched as hub.h launches it): device time
// of ONE k_scale_to_i420_step launch for a step of N device-resident I420 pictures SW x SH -> W x H, by HIP events, against a
// device-to-device hipMemcpyAsync of the same N source pictures in the same process (the copy moves 2 x the source bytes, the
// scaler 1 + W H / (SW SH)).  The two alternate, `reps` times each after a warm-up; prints one JSON line with the medians.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench_scale.bin tools/ubench_scale.hip
// usage: ubench_scale.bin [N SW SH W H [offset]]        (default 16 1920 1080 1280 720 0; offset: bytes the pictures start past 256)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
enum { PIC_I420 = 0, PIC_NV12 = 1, PIC_RGBA = 2 };
#include "../media_amd/csrc/scale_kernels.h"
#define CK(x) do { hipError_t r_ = (x); if (r_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(r_)); exit(1); } } while (0)
int main(int argc, char** argv)
{
    const int n = argc > 5 ? atoi(argv[1]) : 16, sw = argc > 5 ? atoi(argv[2]) : 1920, sh = argc > 5 ? atoi(argv[3]) : 1080;
    const int w = argc > 5 ? atoi(argv[4]) : 1280, h = argc > 5 ? atoi(argv[5]) : 720, off = argc > 6 ? atoi(argv[6]) : 0;
    if (n < 1 || n > 64 || ((sw | sh | w | h) & 1) || w < 16 || h < 16 || sw < w || sh < h || sw > 4 * w || sh > 4 * h || sw > 4096 || sh > 4096 || off < 0 || off > 255) {
        fprintf(stderr, "sizes out of range\n");
        return 2;
    }
    const size_t src_bytes = (size_t)sw * sh * 3 / 2, dst_bytes = (size_t)w * h * 3 / 2;
    const size_t st_src = ((src_bytes + 255) & ~(size_t)255) + 256, st_dst = (dst_bytes + 255) & ~(size_t)255;
    uint8_t *d_src, *d_copy, *d_dst, *d_tab;
    CK(hipMalloc(&d_src, st_src * n)); CK(hipMalloc(&d_copy, st_src * n)); CK(hipMalloc(&d_dst, st_dst * n));
    std::vector<uint8_t> host(st_src * n);
    uint32_t x = 12345;
    for (auto& b : host) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
    CK(hipMemcpy(d_src, host.data(), host.size(), hipMemcpyHostToDevice));
    std::vector<ScaleSrc> tab(n);
    std::vector<unsigned long long> dst(n);
    for (int k = 0; k < n; k++) {
        tab[k] = ScaleSrc{(unsigned long long)(uintptr_t)(d_src + st_src * k + off), (uint32_t)sw, (uint32_t)(sw / 2), PIC_I420, 0};
        dst[k] = (unsigned long long)(uintptr_t)(d_dst + st_dst * k);
    }
    const size_t tab_bytes = n * sizeof(ScaleSrc);
    CK(hipMalloc(&d_tab, tab_bytes + n * 8));
    CK(hipMemcpy(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_tab + tab_bytes, dst.data(), n * 8, hipMemcpyHostToDevice));
    const int th = scale_tile_rows(sh, h);
    const ScalePlane PY = scale_plane_make(sw, sh, w, h), PC = scale_plane_make(sw / 2, sh / 2, w / 2, h / 2);
    const int ntx_y = scale_tiles_x(w, 1), ntx_c = scale_tiles_x(w / 2, 1), nty = (h + th - 1) / th;
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int reps = 50;
    std::vector<float> t_scale, t_copy;
    for (int r = -5; r < reps; r++) {   // (five of each to warm up)
        float ms;
        CK(hipEventRecord(e0, st));
        hipLaunchKernelGGL(k_scale_to_i420_step, dim3((unsigned)(ntx_y + 2 * ntx_c), (unsigned)nty, (unsigned)n), dim3(256), 0, st, (const ScaleSrc*)d_tab,
                           (const unsigned long long*)(d_tab + tab_bytes), 1, PY, PC, ntx_y, ntx_c, th);
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) t_scale.push_back(ms);
        CK(hipEventRecord(e0, st));
        CK(hipMemcpyAsync(d_copy, d_src, st_src * n, hipMemcpyDeviceToDevice, st));
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) t_copy.push_back(ms);
    }
    std::sort(t_scale.begin(), t_scale.end());
    std::sort(t_copy.begin(), t_copy.end());
    const double ms_s = t_scale[reps / 2], ms_c = t_copy[reps / 2];
    const double moved = (double)n * (src_bytes + dst_bytes);
    printf("{\"pictures\": %d, \"source\": \"%dx%d\", \"coded\": \"%dx%d\", \"offset\": %d, \"tile_rows\": %d, \"blocks\": %d, \"scale_ms_median\": %.4f, \"scale_ms_min\": %.4f, "
           "\"scale_ms_max\": %.4f, \"copy_ms_median\": %.4f, \"copy_ms_min\": %.4f, \"copy_ms_max\": %.4f, \"ratio\": %.3f, \"scale_GBps_moved\": %.1f, \"copy_GBps_moved\": %.1f}\n",
           n, sw, sh, w, h, off, th, (ntx_y + 2 * ntx_c) * nty * n, ms_s, t_scale.front(), t_scale.back(), ms_c, t_copy.front(), t_copy.back(), ms_s / ms_c,
           moved / ms_s / 1e6, 2.0 * st_src * n / ms_c / 1e6);
    return 0;
}
