// media_amd/csrc/decoder.h -- the decoder peer (include/mi355x_h264_dec.h): host parser (h264_parse.h) + the reconstruction
// kernels (k_dec.h, k_intra.h, k_deblock.h).  The decoder owns an engine instance for its device buffers (reconstruction ring,
// per-macroblock arrays, hand-off granules, streams): decoding is the encoder's reconstruction path run from parsed decisions.
#pragma once

namespace {

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
mi355x_h264_dec_out_pic out_pic(int64_t off, int w, int h, const OutGeom& g, int fresh, int64_t serial)
{
    mi355x_h264_dec_out_pic p{};
    p.offset = off; p.width = w; p.height = h; p.stride = g.stride; p.chroma_stride = g.cstride; p.fresh = fresh; p.serial = serial;
    return p;
}
mi355x_h264_dec_out_pic out_no_pic(int64_t serial) { mi355x_h264_dec_out_pic p{}; p.offset = -1; p.serial = serial; return p; }

// what the read calls of a decoder or a group own, made with the first call that needs it: the position table in pinned memory
// (the kernel reads it in place: a read call makes no transfer for it) and the staging pair of the host form
struct DecOutBuf {
    DecOutPos* h_tab = nullptr;   // [DEC_GROUP_MAX_STREAMS]
    const DecOutPos* d_tab = nullptr;   // the same memory as the device addresses it
    uint8_t* d_stage = nullptr; size_t d_cap = 0;
    uint8_t* h_stage = nullptr; size_t h_cap = 0;
};
// nothing on the GPU may be using the buffers (the callers have waited for their stream)
hipError_t out_reserve(DevMem& mem, DecOutBuf& b, size_t dev_bytes, size_t host_bytes)
{
    if (!b.h_tab) {
        HIPTRY(mem.pinned(&b.h_tab, 64 * sizeof(DecOutPos)));
        HIPTRY(hipHostGetDevicePointer((void**)&b.d_tab, b.h_tab, 0));
    }
    if (dev_bytes > b.d_cap) {
        if (b.d_stage) mem.drop(b.d_stage);
        b.d_stage = nullptr; b.d_cap = 0;
        HIPTRY(mem.dev(&b.d_stage, dev_bytes));
        b.d_cap = dev_bytes;
    }
    if (host_bytes > b.h_cap) {
        if (b.h_stage) mem.drop(b.h_stage);
        b.h_stage = nullptr; b.h_cap = 0;
        HIPTRY(mem.pinned(&b.h_stage, host_bytes));
        b.h_cap = host_bytes;
    }
    return hipSuccess;
}

// ONE launch for the n pictures of rows[] (d_tab: the same rows as the device reads them) out of engine e's ring into dst
hipError_t launch_dec_out(const mi355x_h264_encoder* e, int layout, const DecOutPos* rows, const DecOutPos* d_tab, int n, uint8_t* dst, hipStream_t st)
{
    int max_bytes = 0, max_rows = 0;
    for (int i = 0; i < n; i++) {
        const int w = (int)rows[i].width, h = (int)rows[i].height;
        max_bytes = std::max(max_bytes, layout == DEC_OUT_RGBA ? 4 * w : w);
        max_rows = std::max(max_rows, layout == DEC_OUT_RGBA ? h : (layout == DEC_OUT_I420 ? h + 2 * (h / 2) : h + h / 2));
    }
    DecOutParams P{};
    P.y = e->d_plane_base[0]; P.u = e->d_plane_base[1]; P.v = e->d_plane_base[2];
    P.st_y = e->st_y; P.st_c = e->st_c; P.st_ring_y = e->st_ring_y; P.st_ring_c = e->st_ring_c;
    P.pitch = e->cw; P.dst = dst; P.tab = d_tab;
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

}  // namespace

struct mi355x_h264_decoder {
    h264dec::Parser parser;
    mi355x_h264_encoder* eng = nullptr;
    int device = 0;
    int mbw = 0, mbh = 0;
    int have_refs = 0;   // reference pictures in the ring (sliding window)
    int max_refs = 1;
    int last = -1;       // ring index of the last decoded picture
    int width = 0, height = 0, crop_x = 0, crop_y = 0;
    uint64_t pictures = 0;
    double parse_ms = 0, gpu_ms = 0;
    uint8_t* d_mbqp = nullptr;   // QP_Y per macroblock of the picture being reconstructed
    int16_t* d_mv4 = nullptr;    // its vectors per 4x4 block (32 int16 per macroblock)
    uint8_t* d_refq = nullptr;   // and reference indices per quadrant (4 per macroblock)
    uint8_t* d_mbavail = nullptr;   // neighbour availability bits per macroblock
    uint32_t* d_lv8 = nullptr;      // the levels as they arrive: one byte each (k_dec_widen fills the engine's int16 lists)
    DevMem mem;                     // the five per-macroblock arrays above (they change with the picture size)
    DecBigLevel* d_big = nullptr;   // levels that did not fit a byte (grows with the largest list met)
    size_t big_cap = 0;
    DecOutBuf out;                  // read in a layout (k_dec_out.h): table and staging, in `mem`
    // One picture of look-ahead: decode() returns once picture n is LAUNCHED; the parse of access unit n + 1 then runs on the
    // host while the GPU reconstructs n.  The parser fills two picture buffers in turn (pinned memory: the uploads are
    // asynchronous); up_done[k] = the uploads out of buffer k have finished, so it may be parsed into again.
    int buf = 0;
    hipEvent_t up_done[2] = {nullptr, nullptr};
    bool up_pending[2] = {false, false};
    bool busy = false;           // a picture is in flight on the engine's stream
    char err[256] = {0};
};

namespace {

double now_ms()
{
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

// the picture in flight has finished (and its wavefront kernels did not time out)
int dec_wait(mi355x_h264_decoder* d)
{
    if (!d->busy) return MI355X_H264_OK;
    d->busy = false;
    mi355x_h264_encoder* e = d->eng;
    HIPCHK(d->err, hipStreamSynchronize(e->stream));
    const int rc = handoff_timeout(e->slots[0].sync, d->err);
    if (rc) d->have_refs = 0;   // that picture is not a usable reference: P pictures are refused until the next IDR
    return rc;
}

// launch the reconstruction of the parsed picture (parser buffer d->buf) into ring slot e->seq.cur; does not wait for it
int dec_submit(mi355x_h264_decoder* d, const h264dec::Picture& pic)
{
    mi355x_h264_encoder* e = d->eng;
    const size_t nmb = (size_t)e->nmb;
    hipStream_t st = e->stream;
    HIPCHK(d->err, hipMemcpyAsync(e->d_mb, pic.mb.data(), nmb * sizeof(MbInfo), hipMemcpyHostToDevice, st));
    HIPCHK(d->err, hipMemcpyAsync(e->d_mvq, pic.mvq.data(), nmb * 16, hipMemcpyHostToDevice, st));
    HIPCHK(d->err, hipMemcpyAsync(e->d_aux, pic.aux.data(), nmb * 16, hipMemcpyHostToDevice, st));
    HIPCHK(d->err, hipMemcpyAsync(d->d_lv8, pic.levels8.data(), nmb * LV_STRIDE, hipMemcpyHostToDevice, st));
    {
        const int words = (int)(nmb * (LV_STRIDE / 4));
        hipLaunchKernelGGL(k_dec_widen, dim3((words + 255) / 256), dim3(256), 0, st, (const uint32_t*)d->d_lv8, (const MbInfo*)e->d_mb, e->d_levels, (int)nmb);
        if (!pic.big.empty()) {
            static_assert(sizeof(h264dec::Picture::Big) == sizeof(DecBigLevel), "layout of the list of large levels");
            if (pic.big.size() > d->big_cap) {
                HIPCHK(d->err, hipStreamSynchronize(st));
                if (d->d_big) (void)hipFree(d->d_big);
                d->d_big = nullptr;
                d->big_cap = pic.big.size() * 2 + 1024;
                HIPCHK(d->err, hipMalloc((void**)&d->d_big, d->big_cap * sizeof(DecBigLevel)));
            }
            HIPCHK(d->err, hipMemcpyAsync(d->d_big, pic.big.data(), pic.big.size() * sizeof(DecBigLevel), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_dec_patch, dim3(((int)pic.big.size() + 255) / 256), dim3(256), 0, st, (const DecBigLevel*)d->d_big, (int)pic.big.size(), e->d_levels);
        }
    }
    HIPCHK(d->err, hipMemcpyAsync(d->d_mbqp, pic.mbqp.data(), nmb, hipMemcpyHostToDevice, st));
    HIPCHK(d->err, hipMemcpyAsync(d->d_mbavail, pic.mbavail.data(), nmb, hipMemcpyHostToDevice, st));
    if (pic.has_inter) {
        HIPCHK(d->err, hipMemcpyAsync(d->d_mv4, pic.mv4.data(), nmb * 64, hipMemcpyHostToDevice, st));
        HIPCHK(d->err, hipMemcpyAsync(d->d_refq, pic.refq.data(), nmb * 4, hipMemcpyHostToDevice, st));
    }
    const int cur = e->seq.cur;
    FrameParams P = frame_params(e);
    P.w = e->cw; P.h = e->ch;
    P.nref = std::max(1, d->have_refs);
    for (int p = 0; p < 3; p++) {
        P.rec[p] = e->d_planes[cur][p];
        for (int r = 0; r < mi355x_h264_encoder::MAX_REFS; r++) {
            // RefPicList0 entry r = the reference picture decoded ref_age[r] + 1 reference pictures ago (ring slot cur - 1 - age)
            const int age = std::min(r < pic.num_ref_active ? pic.ref_age[r] : r, std::max(0, d->have_refs - 1));
            P.refs[r][p] = e->d_planes[(cur + e->nbuf - 1 - age) % e->nbuf][p];
        }
        P.ref[p] = P.refs[0][p];
    }
    // slices that are bands of whole rows run as independent wavefronts; any other shape: one wavefront over the picture (what may
    // be used for prediction is in mbavail either way)
    P.sl.rows = pic.slice_rows > 0 ? pic.slice_rows : e->mbh;
    P.sl.inv = recip32(P.sl.rows);
    P.band.row0 = 0; P.band.rows = e->mbh;
    fill_quant(P.qy, pic.qp);                 // (the reconstruction kernels scale with the macroblock's own QP: mbqp)
    fill_quant(P.qc, h_chroma_qp[pic.qp]);
    P.mbqp = d->d_mbqp; P.cqo_cb = pic.cqo[0]; P.cqo_cr = pic.cqo[1]; P.mv4 = d->d_mv4; P.refq = d->d_refq; P.mbavail = d->d_mbavail;
    {   // the flags the loop filter launches look at: intra macroblocks present (bS 3 / 4 form); I_PCM never switches the filter off here
        const unsigned flags[2] = {0u, pic.has_intra ? P.pic_serial : 0u};
        HIPCHK(d->err, hipMemcpyAsync(e->d_anypcm, &flags[0], sizeof(unsigned), hipMemcpyHostToDevice, st));
        HIPCHK(d->err, hipMemcpyAsync(e->d_anyintra, &flags[1], sizeof(unsigned), hipMemcpyHostToDevice, st));
    }
    HIPCHK(d->err, hipEventRecord(d->up_done[d->buf], st));   // every copy out of the parser's buffer has been queued
    d->up_pending[d->buf] = true;
    unsigned* const h_err = e->slots[0].sync.h_err;
    if (pic.has_inter) {
        hipLaunchKernelGGL(k_dec_inter, dim3(e->nmb, 1), dim3(64), 0, st, P);
        hipLaunchKernelGGL(k_dec_resid<false>, dim3((e->nmb + 3) / 4, 1), dim3(64), 0, st, P);
    }
    if (pic.has_intra) {
        const IntraRowParams R = intra_row_params(e, P, h_err, 1);
        hipLaunchKernelGGL(k_pintra_rows<true>, dim3(e->mbh, 1), dim3(64), 0, st, R);
    }
    if (pic.deblock_idc != 1) {
        // disable_deblocking_filter_idc 0 filters the edges between slices too: the filter then sees one slice
        SliceRows dsl = P.sl;
        // (slices of any other shape than bands: k_dec_bs has zeroed the strengths of the edges between them where idc 2 says so)
        if (pic.deblock_idc == 0 || pic.slice_rows < 0) { dsl.rows = e->mbh; dsl.inv = recip32(e->mbh); }
        const unsigned db_serial = next_nonzero(e->serial);
        {   // vectors per 4x4 block, references per quadrant, slice edges from the availability bits
            DecBsParams B{};
            B.mb = e->d_mb; B.mv4 = d->d_mv4; B.refq = d->d_refq; B.bs = (uint8_t*)e->d_bs; B.mbw = e->mbw; B.nmb = e->nmb; B.mbdiv = P.mbdiv;
            B.mbavail = d->d_mbavail; B.across = pic.deblock_idc == 0;
            hipLaunchKernelGGL(k_dec_bs, dim3((e->nmb + 1) / 2, 1), dim3(64), 0, st, B, e->d_anybs, db_serial);
        }
        DbParams D = db_params(e, e->d_planes[cur], dsl, pic.qp);
        D.mbqp = d->d_mbqp; D.oa = pic.filter_oa; D.ob = pic.filter_ob; D.cqo_cb = pic.cqo[0]; D.cqo_cr = pic.cqo[1];
        DbRowParams R = db_row_params(e, D, h_err, db_serial, P.pic_serial, 0, 1);
        // one_qp: the per-picture thresholds above are every edge's (the encoder's own streams); else per edge from mbqp
        if (!pic.one_qp) {
            R.need_intra = 0;
            if (pic.has_intra) hipLaunchKernelGGL((k_deblock_rows<true, true>), dim3(e->mbh, 1), dim3(64), 0, st, R);
            else hipLaunchKernelGGL((k_deblock_rows<false, true>), dim3(e->mbh, 1), dim3(64), 0, st, R);
        } else if (!pic.has_inter) { R.need_intra = 0; hipLaunchKernelGGL(k_deblock_rows<true>, dim3(e->mbh, 1), dim3(64), 0, st, R); }
        else {
            R.need_intra = -1; hipLaunchKernelGGL(k_deblock_rows<false>, dim3(e->mbh, 1), dim3(64), 0, st, R);
            R.need_intra = 1; hipLaunchKernelGGL(k_deblock_rows<true>, dim3(e->mbh, 1), dim3(64), 0, st, R);
        }
    }
    HIPCHK(d->err, hipGetLastError());
    d->busy = true;
    return MI355X_H264_OK;
}

void* pinned_alloc(size_t n)
{
    void* p = nullptr;
    return hipHostMalloc(&p, n, hipHostMallocPortable) == hipSuccess ? p : nullptr;
}
void pinned_free(void* p) { (void)hipHostFree(p); }

int dec_decode_unit(mi355x_h264_decoder* d, const uint8_t* au, size_t len, int* got_picture)
{
    if (!d || !au) return MI355X_H264_E_ARG;
    if (got_picture) *got_picture = 0;
    d->err[0] = 0;
    if (hipSetDevice(d->device) != hipSuccess) return set_err(d->err, MI355X_H264_E_HIP, "hipSetDevice");
    // parse into the buffer the picture in flight does NOT come from (its uploads, two pictures back, have long finished)
    const int k = d->buf ^ 1;
    if (d->up_pending[k]) { HIPCHK(d->err, hipEventSynchronize(d->up_done[k])); d->up_pending[k] = false; }
    d->parser.select(k);
    const double t0 = now_ms();
    const int rc = d->parser.parse_access_unit(au, len, false);   // (the picture enters the parser's reference list below, once launched)
    const double t1 = now_ms();
    d->parse_ms += t1 - t0;
    if (rc <= 0) d->parser.select(d->buf);   // nothing to launch: picture() stays the last good one
    if (rc < 0) return set_err(d->err, MI355X_H264_E_STREAM, "%s", d->parser.error().c_str());
    if (rc == 0) return MI355X_H264_OK;
    // the picture in flight must be out of the way before this one is launched (one picture of look-ahead, and its time-out
    // flag is checked here)
    if (const int wrc = dec_wait(d)) return wrc;
    d->buf = k;
    const h264dec::Picture& pic = d->parser.picture();
    const h264dec::Sps& sps = d->parser.sps();
    if (!d->eng || d->mbw != pic.mbw || d->mbh != pic.mbh) {
        if (!pic.idr) return set_err(d->err, MI355X_H264_E_STREAM, "the stream must start with an IDR picture");
        if (d->eng) { destroy_engine(d->eng); d->eng = nullptr; }
        mi355x_h264_config cfg;
        mi355x_h264_default_config(&cfg);
        cfg.width = 16 * pic.mbw; cfg.height = 16 * pic.mbh; cfg.refs = 3; cfg.device = d->device; cfg.batch = 1;
        const int crc = create_engine(&cfg, &d->eng, false);
        if (crc != MI355X_H264_OK) return set_err(d->err, crc, "engine for %dx%d macroblocks could not be created", pic.mbw, pic.mbh);
        d->mbw = pic.mbw; d->mbh = pic.mbh; d->have_refs = 0; d->last = -1;
        d->mem.free_all();   // (a picture after an allocation that failed below must meet null pointers, not the freed arrays)
        d->d_mbqp = d->d_refq = d->d_mbavail = nullptr; d->d_mv4 = nullptr; d->d_lv8 = nullptr;
        d->out = DecOutBuf();
        const size_t n = (size_t)pic.mbw * pic.mbh;
        if (d->mem.dev(&d->d_mbqp, n) != hipSuccess || d->mem.dev(&d->d_mv4, n * 64) != hipSuccess || d->mem.dev(&d->d_refq, n * 4) != hipSuccess ||
            d->mem.dev(&d->d_mbavail, n) != hipSuccess || d->mem.dev(&d->d_lv8, n * LV_STRIDE) != hipSuccess)
            return set_err(d->err, MI355X_H264_E_NOMEM, "hipMalloc (per-macroblock decoder arrays)");
    }
    d->width = pic.width; d->height = pic.height; d->crop_x = 2 * sps.crop_l; d->crop_y = 2 * sps.crop_t;
    d->max_refs = std::max(1, sps.max_refs);
    if (pic.idr) d->have_refs = 0;
    if (pic.has_inter && (d->have_refs < 1 || pic.num_ref_active > d->have_refs))
        return set_err(d->err, MI355X_H264_E_STREAM, "a P picture refers to %d reference pictures, %d are held", pic.num_ref_active, d->have_refs);
    for (int r = 0; pic.has_inter && r < pic.num_ref_active && r < 3; r++)
        if (pic.ref_age[r] < 0 || pic.ref_age[r] >= d->have_refs) return set_err(d->err, MI355X_H264_E_STREAM, "reference list entry %d is not a held picture", r);
    int src = dec_submit(d, pic);
    static const bool no_lookahead = getenv("MI355X_H264_DEC_SYNC") != nullptr;   // (measurements: wait for every picture before returning)
    if (src == MI355X_H264_OK && no_lookahead) src = dec_wait(d);
    d->gpu_ms += now_ms() - t1;
    if (src != MI355X_H264_OK) return src;
    d->last = d->eng->seq.cur;
    d->parser.commit();   // parser and ring take the picture in together
    if (pic.is_ref) {   // sliding window (8.2.5.3)
        d->eng->seq.cur = (d->eng->seq.cur + 1) % d->eng->nbuf;
        d->have_refs = std::min(d->have_refs + 1, std::min(d->max_refs, d->eng->nrefs));
    }
    d->pictures++;
    if (got_picture) *got_picture = 1;
    return MI355X_H264_OK;
}

int64_t dec_read(mi355x_h264_decoder* d, void* dst, size_t cap, bool to_device)
{
    if (!d || !dst || d->last < 0) return MI355X_H264_E_ARG;
    const size_t w = (size_t)d->width, h = (size_t)d->height, need = w * h * 3 / 2;
    if (cap < need) return MI355X_H264_E_ARG;
    if (hipSetDevice(d->device) != hipSuccess) return set_err(d->err, MI355X_H264_E_HIP, "hipSetDevice");
    if (const int wrc = dec_wait(d)) return wrc;   // the picture asked for may still be in flight
    const mi355x_h264_encoder* e = d->eng;
    uint8_t* o = (uint8_t*)dst;
    const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int p = 0; p < 3; p++) {
        const size_t pw = p ? w / 2 : w, ph = p ? h / 2 : h, pitch = p ? (size_t)e->cw / 2 : (size_t)e->cw;
        const uint8_t* s = e->d_planes[d->last][p] + (size_t)(p ? d->crop_y / 2 : d->crop_y) * pitch + (size_t)(p ? d->crop_x / 2 : d->crop_x);
        if (hipMemcpy2D(o, pw, s, pitch, pw, ph, kind) != hipSuccess) return set_err(d->err, MI355X_H264_E_HIP, "hipMemcpy2D");
        o += pw * ph;
    }
    return (int64_t)need;
}

// the last picture in a layout: the group's kernel with one position (batch item 0, ring slot `last`)
int64_t dec_read_out(mi355x_h264_decoder* d, int layout, int row_align, void* dst, size_t cap, bool to_device, mi355x_h264_dec_out_pic* pic)
{
    if (!d || !pic || !out_args_ok(layout, row_align) || d->last < 0) return MI355X_H264_E_ARG;
    const OutGeom geo = out_geom(layout, d->width, d->height, row_align);
    if (dst && (cap < geo.bytes || (to_device && ((uintptr_t)dst & 15)))) return MI355X_H264_E_ARG;
    *pic = out_pic(0, d->width, d->height, geo, 1, (int64_t)d->pictures);
    if (!dst) return (int64_t)geo.bytes;
    if (hipSetDevice(d->device) != hipSuccess) return set_err(d->err, MI355X_H264_E_HIP, "hipSetDevice");
    if (const int wrc = dec_wait(d)) return wrc;   // the picture asked for may still be in flight
    const mi355x_h264_encoder* e = d->eng;
    const size_t stage = to_device ? 0 : geo.bytes;
    if (out_reserve(d->mem, d->out, stage, stage) != hipSuccess) return set_err(d->err, MI355X_H264_E_NOMEM, "memory for the output staging (%s)", t_failed_call);
    d->out.h_tab[0] = DecOutPos{0u, (uint32_t)d->last, (uint32_t)d->crop_x, (uint32_t)d->crop_y, (uint32_t)d->width, (uint32_t)d->height,
                                (uint32_t)geo.stride, (uint32_t)geo.cstride, 0ull, 0ull};
    HIPCHK(d->err, launch_dec_out(e, layout, d->out.h_tab, d->out.d_tab, 1, to_device ? (uint8_t*)dst : d->out.d_stage, e->stream));
    if (!to_device) HIPCHK(d->err, hipMemcpyAsync(d->out.h_stage, d->out.d_stage, geo.bytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(d->err, hipStreamSynchronize(e->stream));
    if (!to_device) memcpy(dst, d->out.h_stage, geo.bytes);
    return (int64_t)geo.bytes;
}

}  // namespace
