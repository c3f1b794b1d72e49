// media_amd/csrc/dec_out.h -- host side of k_dec_out.h and k_dec_out_scale.h: the geometry of a picture in a layout
// (include/mi355x_h264_dec.h states the packing), the output size of a stream, the table and staging buffers of the read calls,
// and the ONE launch that serves them (dec_group.h).
#pragma once

namespace {

double now_ms()
{
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

// ---- output in a layout (k_dec_out.h; include/mi355x_h264_dec.h states the packing) ----
struct OutGeom { int stride, cstride; size_t bytes; };
bool out_args_ok(int layout, int row_align) { return layout >= 0 && layout <= 3 && row_align >= 1 && row_align <= 256 && (row_align & (row_align - 1)) == 0; }
size_t out_align(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
OutGeom out_geom(int layout, int w, int h, int row_align)
{
    const size_t a = (size_t)row_align;
    OutGeom g{};
    if (layout == DEC_OUT_RGBA) { g.stride = (int)out_align(4 * (size_t)w, a); g.bytes = (size_t)g.stride * h; }
    else if (layout == DEC_OUT_I420) { g.stride = (int)out_align(w, a); g.cstride = (int)out_align(w / 2, a); g.bytes = (size_t)g.stride * h + 2 * (size_t)g.cstride * (h / 2); }
    else { g.stride = g.cstride = (int)out_align(w, a); g.bytes = (size_t)g.stride * h + (size_t)g.cstride * (h / 2); }
    return g;
}
// variant: of the RGBA conversion that is applied to the picture (k_dec_out.h), -1 for the other layouts; the picture's `colour`
// names it as matrix | full_range << 8 with the matrix code of the variant's numbers (6 for a stream that says 5)
mi355x_h264_dec_out_pic out_pic(int64_t off, int w, int h, const OutGeom& g, int fresh, int64_t serial, int variant)
{
    mi355x_h264_dec_out_pic p{};
    p.offset = off; p.width = w; p.height = h; p.stride = g.stride; p.chroma_stride = g.cstride; p.fresh = fresh; p.serial = serial;
    p.colour = variant < 0 ? 0 : ((variant & 1) ? MI355X_H264_MATRIX_BT709 : MI355X_H264_MATRIX_BT601) | ((variant >> 1) << 8);
    return p;
}
mi355x_h264_dec_out_pic out_no_pic(int64_t serial) { mi355x_h264_dec_out_pic p{}; p.offset = -1; p.serial = serial; return p; }

// ---- output size (include/mi355x_h264_dec.h, "output size"; k_dec_out_scale.h) ----
// what set_output_size takes: (0, 0) = the native size, else both even and 2..4096
bool out_size_ok(int W, int H)
{
    if (W == 0 && H == 0) return true;
    return W >= 2 && W <= 4096 && H >= 2 && H <= 4096 && !(W & 1) && !(H & 1);
}
// a picture of w x h can be resampled to W x H: no upscaling, no ratio above 4
bool out_size_serves(int w, int h, int W, int H) { return W <= w && w <= 4 * W && H <= h && h <= 4 * H; }
// the scaled form of a table row whose width / height are the RESULT size, for a cropped picture of w x h.  The tile height: as many
// result rows as SC_ROWS source rows serve (scale_tile_rows), even, so that a tile's chroma rows are its own
DecOutScalePos out_scale_pos(const DecOutPos& o, int w, int h)
{
    DecOutScalePos t{};
    t.o = o;
    t.y = scale_plane_make(w, h, (int)o.width, (int)o.height);
    t.c = scale_plane_make(w / 2, h / 2, (int)o.width / 2, (int)o.height / 2);
    t.th = (uint32_t)std::min((int)DOS_TH, scale_tile_rows(h, (int)o.height) & ~1);
    return t;
}

// what the read calls of a decoder or a group own, made with the first call that needs it: the position table in pinned memory
// (the kernel reads it in place: a read call makes no transfer for it) and the staging pair of the host form
struct DecOutBuf {
    uint8_t* h_tab = nullptr;     // [DEC_GROUP_MAX_STREAMS] rows: DecOutPos, or DecOutScalePos when a position of the call is scaled
    const uint8_t* d_tab = nullptr;     // the same memory as the device addresses it
    uint8_t* d_stage = nullptr; size_t d_cap = 0;
    uint8_t* h_stage = nullptr; size_t h_cap = 0;
};
// nothing on the GPU may be using the buffers (the callers have waited for their stream)
hipError_t out_reserve(DevMem& mem, DecOutBuf& b, size_t dev_bytes, size_t host_bytes)
{
    if (!b.h_tab) {
        HIPTRY(DM_PINNED(mem, b.h_tab, 64 * sizeof(DecOutScalePos)));
        HIPTRY(hipHostGetDevicePointer((void**)&b.d_tab, b.h_tab, 0));
    }
    if (dev_bytes > b.d_cap) {
        if (b.d_stage) mem.drop(b.d_stage);
        b.d_stage = nullptr; b.d_cap = 0;
        HIPTRY(DM_DEV(mem, b.d_stage, dev_bytes, false));
        b.d_cap = dev_bytes;
    }
    if (host_bytes > b.h_cap) {
        if (b.h_stage) mem.drop(b.h_stage);
        b.h_stage = nullptr; b.h_cap = 0;
        HIPTRY(DM_PINNED(mem, b.h_stage, host_bytes));
        b.h_cap = host_bytes;
    }
    return hipSuccess;
}

// ONE launch for the n pictures of rows[] (d_tab: the same rows as the device reads them) out of the store's ring into dst
hipError_t launch_dec_out(const PicStore* s, int layout, const DecOutPos* rows, const DecOutPos* d_tab, int n, uint8_t* dst, hipStream_t st)
{
    int max_bytes = 0, max_rows = 0;
    for (int i = 0; i < n; i++) {
        const int w = (int)rows[i].width, h = (int)rows[i].height;
        max_bytes = std::max(max_bytes, layout == DEC_OUT_RGBA ? 4 * w : w);
        max_rows = std::max(max_rows, layout == DEC_OUT_RGBA ? h : (layout == DEC_OUT_I420 ? h + 2 * (h / 2) : h + h / 2));
    }
    DecOutParams P{};
    P.y = s->d_plane_base[0]; P.u = s->d_plane_base[1]; P.v = s->d_plane_base[2];
    P.st_y = s->st_y; P.st_c = s->st_c; P.st_ring_y = s->st_ring_y; P.st_ring_c = s->st_ring_c;
    P.pitch = s->cw; P.dst = dst; P.tab = d_tab;
    // a row of b bytes that starts anywhere touches at most b / 16 + 2 chunks of 16 aligned bytes
    const dim3 grid((unsigned)((max_bytes / 16 + 2 + 63) / 64), (unsigned)((max_rows + 4 * DEC_OUT_ROWS - 1) / (4 * DEC_OUT_ROWS)), (unsigned)n), block(64, 4);
    switch (layout) {
        case DEC_OUT_I420: hipLaunchKernelGGL(k_dec_out<DEC_OUT_I420>, grid, block, 0, st, P); break;
        case DEC_OUT_NV12: hipLaunchKernelGGL(k_dec_out<DEC_OUT_NV12>, grid, block, 0, st, P); break;
        case DEC_OUT_NV21: hipLaunchKernelGGL(k_dec_out<DEC_OUT_NV21>, grid, block, 0, st, P); break;
        default: hipLaunchKernelGGL(k_dec_out<DEC_OUT_RGBA>, grid, block, 0, st, P); break;
    }
    return hipGetLastError();
}

// the same for a call with at least one scaled position: ONE launch of k_dec_out_scaled for all n rows
hipError_t launch_dec_out_scaled(const PicStore* s, int layout, const DecOutScalePos* rows, const DecOutScalePos* d_tab, int n, uint8_t* dst, hipStream_t st)
{
    int tx = 1, ty = 1;
    for (int i = 0; i < n; i++) {
        tx = std::max(tx, ((int)rows[i].o.width + DOS_TW - 1) / DOS_TW);
        ty = std::max(ty, ((int)rows[i].o.height + (int)rows[i].th - 1) / (int)rows[i].th);
    }
    DecOutParams P{};
    P.y = s->d_plane_base[0]; P.u = s->d_plane_base[1]; P.v = s->d_plane_base[2];
    P.st_y = s->st_y; P.st_c = s->st_c; P.st_ring_y = s->st_ring_y; P.st_ring_c = s->st_ring_c;
    P.pitch = s->cw; P.dst = dst; P.tab = nullptr;
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)n), block(256);
    switch (layout) {
        case DEC_OUT_I420: hipLaunchKernelGGL(k_dec_out_scaled<DEC_OUT_I420>, grid, block, 0, st, P, d_tab); break;
        case DEC_OUT_NV12: hipLaunchKernelGGL(k_dec_out_scaled<DEC_OUT_NV12>, grid, block, 0, st, P, d_tab); break;
        case DEC_OUT_NV21: hipLaunchKernelGGL(k_dec_out_scaled<DEC_OUT_NV21>, grid, block, 0, st, P, d_tab); break;
        default: hipLaunchKernelGGL(k_dec_out_scaled<DEC_OUT_RGBA>, grid, block, 0, st, P, d_tab); break;
    }
    return hipGetLastError();
}

// What a call delivers, as its table is made: rows[] with width / height = the size DELIVERED, src[] the cropped size of each picture,
// scaled = at least one stream of the call has an output size.  out_fill writes the table the kernel reads into `tab` (pinned: read
// in place, or sent along with the step's position table) and returns its bytes; out_launch makes the ONE launch from that table:
// k_dec_out as ever when no position is scaled, else k_dec_out_scaled for all of them (native positions: ratio 1)
struct OutCall {
    DecOutPos rows[DEC_GROUP_MAX_STREAMS];
    int src[DEC_GROUP_MAX_STREAMS][2];
    int n = 0;
    bool scaled = false;
};
size_t out_fill(const OutCall& c, uint8_t* tab)
{
    if (!c.scaled) { memcpy(tab, c.rows, (size_t)c.n * sizeof(DecOutPos)); return (size_t)c.n * sizeof(DecOutPos); }
    DecOutScalePos* const t = (DecOutScalePos*)tab;
    for (int i = 0; i < c.n; i++) t[i] = out_scale_pos(c.rows[i], c.src[i][0], c.src[i][1]);
    return (size_t)c.n * sizeof(DecOutScalePos);
}
hipError_t out_launch(const PicStore* s, int layout, const OutCall& c, const uint8_t* tab, const uint8_t* d_tab, uint8_t* dst, hipStream_t st)
{
    if (!c.scaled) return launch_dec_out(s, layout, c.rows, (const DecOutPos*)d_tab, c.n, dst, st);
    return launch_dec_out_scaled(s, layout, (const DecOutScalePos*)tab, (const DecOutScalePos*)d_tab, c.n, dst, st);
}

}  // namespace
