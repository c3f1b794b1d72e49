// media_amd/csrc/hub.h -- the stream hub's HIP side (include/mi355x_h264.h, "streams"): streams of one geometry share an engine
// whose batch items are the streams; the pictures that calls deliver while the engine is busy leave together as ONE lockstep
// step (the IND = true kernels).  The engine searches config.refs reference pictures and keeps refs + 1 reconstructions per stream
// slot ((refs + 1) * cap * 1.5 * coded size bytes: at 1920x1088 with 32 slots 200 / 300 / 400 MB for refs 1 / 2 / 3); every position
// of a step has its own number of usable ones (ItemPic.nref).  Who gathers, leads and waits is hub_sched.h; here: staging memory, uploads, the step itself.
#pragma once

namespace {

static_assert(HUB_MAX_ITEMS == MAX_BATCH, "a hub's streams are the batch items of its engine");

enum { HUB_IN_DEVICE = 3 };   // HostPicture.layout of a stream call that was handed one tight device picture in the stream's layout
static_assert(PIC_I420 == MI355X_H264_INPUT_I420 && PIC_NV12 == MI355X_H264_INPUT_NV12 && PIC_RGBA == MI355X_H264_INPUT_RGBA, "layouts");

// the device side of a stream: its request in flight and the answer
struct HubItem {
    hipEvent_t copied = nullptr;     // the picture's upload has finished
    // where the picture lies.  staged: it was uploaded to the item's staging slot (`copied` says when it has arrived); else d_in is
    // the caller's own device picture, read in place.  RGBA pictures (rgba_src, rgba_stride: the caller's device picture or the
    // item's RGBA staging slot) are converted into the I420 staging slot by the step's leader.
    bool staged = true;
    const uint8_t* d_in = nullptr;
    const uint8_t* rgba_src = nullptr;
    size_t rgba_stride = 0;
    // scaling hubs: the tight source picture (the caller's device picture or the item's source staging slot); the step's scaler
    // writes the I420 staging slot (RGBA: the item's RGBA staging slot, which the conversion launch then reads)
    const uint8_t* scale_src = nullptr;
    // damage tiles (damage.h).  slot_valid: the stream's staging slot and its pinned twin hold the stream's last picture - set by a
    // host call that succeeded, clear at open, after a device-form call and after a call that failed (a failed upload or step
    // leaves the twin written and the slot partly or not: they may differ).  patch_tiles: tiles of this call's payload, which the
    // step's patch launch writes into the slot (0: none).  up_*: mi355x_h264_stream_last_upload.  mark: scratch, one byte per tile
    bool slot_valid = false;
    uint32_t patch_tiles = 0;
    uint64_t up_bytes = 0;
    uint32_t up_tiles = 0;
    int up_mode = damage::MODE_WHOLE;
    std::vector<uint8_t> mark;
    int rc = 0, frame_type = 0;
    uint8_t* out = nullptr;
    uint32_t out_len = 0;
    char err[256] = {0};
};

struct HubCtx {
    StepSync sync;                   // a stream pair of its own
    // the step's tables, one pinned block and one transfer: [source address per position][itemtab word per position][RGBA hubs:
    // {address, row stride}][scaling hubs: ScaleSrc per position][steps with damage tiles: PatchSrc per picture that has some]
    enum { TAB_SRC = 0, TAB_ITEM = MAX_BATCH * 8, TAB_RGBA = TAB_ITEM + MAX_BATCH * 4, TAB_SCALE = TAB_RGBA + MAX_BATCH * 16,
           TAB_PATCH = TAB_SCALE + MAX_BATCH * (int)sizeof(ScaleSrc), TAB_BYTES = TAB_PATCH + MAX_BATCH * (int)sizeof(PatchSrc) };
    uint8_t* h_tab = nullptr;        // pinned
    uint8_t* d_tab = nullptr;
};

struct Hub {
    HubSched sched;                  // queue, item states, step contexts: sched.mu guards them
    std::mutex launch_mu;            // one leader at a time touches the engine's host state (serials, statistics)
    mi355x_h264_encoder* e = nullptr;
    mi355x_h264_config cfg{};
    DevMem mem;
    HubItem items[MAX_BATCH];
    HubCtx ctx[HUB_MAX_CTX];         // ctx[0 .. nctx_p - 1] take the P steps, ctx[nctx_p] the IDR steps
    int fmt = MI355X_H264_INPUT_I420;   // layout of every picture of this hub's streams (config.input_format)
    ColourDesc colour;               // the description of every stream of this hub (mi355x_h264_stream_open_colour); the engine's parameter sets carry it
    uint8_t* d_stage = nullptr;      // [cap] pictures the kernels read when the caller's are not read in place: host pictures as handed
    uint8_t* h_stage = nullptr;      // over (tight I420 / NV12; pinned h_stage on their way), RGBA pictures after the conversion (I420)
    size_t st_stage = 0;
    uint8_t* d_rgba = nullptr;       // [cap] host RGBA pictures on their way to the conversion kernel: allocated with the hub's
    uint8_t* h_rgba = nullptr;       // first one (pinned)
    size_t st_rgba = 0;
    // scaling hubs (mi355x_h264_stream_open_scaled): pictures arrive sw x sh and the step's scaler resamples them to cfg.width x
    // cfg.height.  d_src / h_src: [cap] host pictures of the source size on their way to it, allocated with the hub's first one;
    // RGBA: d_rgba holds the [cap] RESAMPLED RGBA pictures (device only, allocated with the hub)
    int sw = 0, sh = 0;              // the size of the pictures the calls take (an ordinary hub: cfg.width, cfg.height)
    bool scaled = false;
    uint8_t* d_src = nullptr;
    uint8_t* h_src = nullptr;
    size_t st_src = 0;
    // damage tiles: [cap] payloads (damage.h: header, tile indices, tiles) on their way to the step's patch launch, st_src apart (a
    // payload that goes is smaller than the picture); allocated with the hub's first damage call
    uint8_t* d_patch = nullptr;
    uint8_t* h_patch = nullptr;
    std::atomic<uint64_t> patch_launches{0}, patch_tiles{0};   // k_patch_step launches of this hub and the tiles they wrote (test hook)
    // uploads: item k on copy stream k % NCOPY.  Two streams fill most of the link (tools/ubench_h2d.hip: 1 stream 32 GB/s, 2: 46-51,
    // 4+: 52-57); HIP streams are a scarce resource on this runtime - beyond about a dozen live streams in the process every launch
    // gets slower (measured: 8 copy streams per hub halved the throughput at 64 streams)
    enum { NCOPY = 2 };
    hipStream_t copy_st[NCOPY] = {nullptr};
    // where a picture's time goes (microseconds, summed; MI355X_H264_HUB_VERBOSE=1 prints them when the hub is freed)
    std::atomic<uint64_t> us_upload{0}, us_launch{0}, us_gpu{0}, us_finish{0}, us_total{0};
    bool verbose = false;
};

std::mutex g_hubs_mu;
std::vector<Hub*> g_hubs;
std::atomic<int> g_streams_open{0};   // over all hubs of the process

// (refs: 0 and 1 are both one reference picture; streams that search more have rings of another size, so engines of their own)
// (colour: the parameter sets are the engine's, so a described stream shares one only with streams of its description)
// (refresh: a hub of intra refresh streams launches the other form of k_me - never shared with ordinary streams of as many slices)
bool same_geometry(const Hub& hub, const mi355x_h264_config& b, int sw, int sh, const ColourDesc& colour, bool refresh)
{
    const mi355x_h264_config& a = hub.cfg;
    return (hub.e->shape.refresh != 0) == refresh && same_colour(hub.colour, colour) && hub.sw == sw && hub.sh == sh && std::max(a.refs, 1) == std::max(b.refs, 1) && a.width == b.width && a.height == b.height && a.fps == b.fps && a.profile_idc == b.profile_idc && a.device == b.device &&
           a.disable_deblock == b.disable_deblock && a.slices == b.slices && a.search == b.search && a.input_format == b.input_format;
}

void hub_free(Hub* h)
{
    if (!h) return;
    HubSched& S = h->sched;
    (void)hipSetDevice(h->cfg.device);
    for (auto& c : h->ctx) sync_destroy(c.sync);
    for (auto& cs : h->copy_st) if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    for (auto& it : h->items) if (it.copied) (void)hipEventDestroy(it.copied);
    h->mem.free_all();
    if (h->verbose && S.pictures)
        fprintf(stderr, "mi355x_h264 hub %dx%d: %llu pictures in %llu steps (%.2f per step, largest %llu); per picture: upload %.0f us, queued %.0f us, "
                        "whole call %.0f us; per step: launch %.0f us, GPU wait %.0f us, finish %.0f us\n", h->cfg.width, h->cfg.height,
                (unsigned long long)S.pictures, (unsigned long long)S.steps, (double)S.pictures / S.steps, (unsigned long long)S.max_batch,
                (double)h->us_upload / S.pictures, (double)S.us_queue / S.pictures, (double)h->us_total / S.pictures,
                (double)h->us_launch / S.steps, (double)h->us_gpu / S.steps, (double)h->us_finish / S.steps);
    if (h->e) destroy_engine(h->e);
    delete h;
}

hipError_t hub_alloc(Hub* h)
{
    HIPTRY(hipSetDevice(h->cfg.device));
    h->mem.configure();
    HIPTRY(DM_DEV(h->mem, h->d_stage, h->st_stage * h->sched.cap, false));
    HIPTRY(DM_PINNED(h->mem, h->h_stage, h->st_stage * h->sched.cap));
    if (h->scaled && h->fmt == MI355X_H264_INPUT_RGBA) HIPTRY(DM_DEV(h->mem, h->d_rgba, h->st_rgba * h->sched.cap, false));
    for (auto& cs : h->copy_st) HIPTRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    const char* one = getenv("MI355X_H264_ONE_STREAM");
    for (int ci = 0; ci <= h->sched.nctx_p; ci++) {
        HubCtx& c = h->ctx[ci];
        // (the IDR context has one stream: its row wavefront dominates, nothing to overlap)
        HIPTRY(sync_create(c.sync, nullptr, nullptr, (one && one[0] == '1') || ci == h->sched.nctx_p));
        HIPTRY(DM_PINNED(h->mem, c.h_tab, HubCtx::TAB_BYTES));
        HIPTRY(DM_DEV(h->mem, c.d_tab, HubCtx::TAB_BYTES, false));
    }
    for (int i = 0; i < h->sched.cap; i++) HIPTRY(hipEventCreateWithFlags(&h->items[i].copied, hipEventDisableTiming));
    return hipSuccess;
}

int hub_create(const mi355x_h264_config& cfg, int sw, int sh, const ColourDesc& colour, bool refresh, Hub** out)
{
    Hub* h = new (std::nothrow) Hub();
    if (!h) return MI355X_H264_E_NOMEM;
    h->cfg = cfg;
    h->colour = colour;
    h->fmt = cfg.input_format;
    h->sw = sw; h->sh = sh; h->scaled = sw != cfg.width || sh != cfg.height;
    const char* ci = getenv("MI355X_H264_HUB_ITEMS");
    h->sched.cap = std::min((int)MAX_BATCH, std::max(1, ci ? atoi(ci) : 32));
    const char* wu = getenv("MI355X_H264_HUB_WINDOW_US");
    if (wu) h->sched.window_us = std::max(0, atoi(wu));
    h->verbose = getenv("MI355X_H264_HUB_VERBOSE") != nullptr;
    // MI355X_H264_HUB_CTX = contexts for P steps (default 2, 1..8): one step's loop filter overlaps the other's motion search.  More
    // contexts mean more HIP streams, and those cost more than they bring (measured: 4 contexts -5 %, 6 contexts -50 %)
    const char* nc = getenv("MI355X_H264_HUB_CTX");
    h->sched.nctx_p = std::min((int)HUB_MAX_CTX - 1, std::max(1, nc ? atoi(nc) : 2));
    mi355x_h264_config ec = cfg;
    ec.batch = h->sched.cap; ec.refs = std::max(cfg.refs, 1); ec.band_index = 0; ec.band_count = 0; ec.input_format = MI355X_H264_INPUT_I420;
    int rc = create_engine(&ec, &h->e, true, &h->colour, cfg.input_format == MI355X_H264_INPUT_RGBA);
    if (rc != MI355X_H264_OK) { h->e = nullptr; hub_free(h); return rc; }
    h->e->shape.refresh = refresh ? 1 : 0;   // (no byte of the parameter sets depends on it: set behind their making)
    h->sched.nrefs = h->e->nrefs; h->sched.nbuf = h->e->nbuf;   // (up to 4 ring slots: `cur` fits the itemtab word's two bits)
    h->st_stage = (picture_bytes(PIC_I420, cfg.width, cfg.height) + 255) & ~(size_t)255;
    h->st_rgba = (picture_bytes(PIC_RGBA, cfg.width, cfg.height) + 255) & ~(size_t)255;
    h->st_src = (picture_bytes(h->fmt, sw, sh) + 255) & ~(size_t)255;
    if (hub_alloc(h) != hipSuccess) { hub_free(h); return MI355X_H264_E_HIP; }
    *out = h;
    return MI355X_H264_OK;
}

// one lockstep step for the gathered pictures T (all of one type) on context T.ctx: launch, wait, finish; rc[k] answers
void hub_run_step(Hub* h, HubStep& T)
{
    mi355x_h264_encoder* e = h->e;
    HubCtx& c = h->ctx[T.ctx];
    StepSync& Y = c.sync;
    (void)hipSetDevice(h->cfg.device);
    const int n = T.n; const bool idr = T.idr;
    const ItemPic* const pics = T.picks;
    Step St;
    int rc = MI355X_H264_OK;
    char errtxt[256] = {0};
    const uint64_t t0 = now_us();
    {
        std::lock_guard<std::mutex> lk(h->launch_mu);
        const bool rgba = h->fmt == MI355X_H264_INPUT_RGBA;
        unsigned long long* const h_src = (unsigned long long*)(c.h_tab + HubCtx::TAB_SRC);
        uint32_t* const h_itemtab = (uint32_t*)(c.h_tab + HubCtx::TAB_ITEM);
        RgbaSrc* const h_rgbatab = (RgbaSrc*)(c.h_tab + HubCtx::TAB_RGBA);
        ScaleSrc* const h_scaletab = (ScaleSrc*)(c.h_tab + HubCtx::TAB_SCALE);
        const bool scaled = h->scaled;
        PatchSrc* const h_patchtab = (PatchSrc*)(c.h_tab + HubCtx::TAB_PATCH);
        int npatch = 0;
        uint32_t patch_most = 0, patch_sum = 0;
        for (int k = 0; k < n; k++) {
            const HubItem& it = h->items[pics[k].item];
            bool bad = false;
            h_itemtab[k] = item_word(pics[k], &bad);
            if (bad) rc = set_err(e->err, MI355X_H264_E_INTERNAL, "step position %d: a fact of the picture does not fit the itemtab word", k);
            // the picture the kernels read: the caller's own (read where it lies), or the item's staging slot
            h_src[k] = (unsigned long long)(uintptr_t)(it.d_in ? it.d_in : h->d_stage + (size_t)pics[k].item * h->st_stage);
            // (a scaling RGBA hub: the conversion reads the item's slot of the resampled RGBA pictures)
            if (rgba && scaled) h_rgbatab[k] = RgbaSrc{(unsigned long long)(uintptr_t)(h->d_rgba + (size_t)pics[k].item * h->st_rgba), (unsigned long long)h->cfg.width * 4};
            else if (rgba) h_rgbatab[k] = RgbaSrc{(unsigned long long)(uintptr_t)it.rgba_src, (unsigned long long)it.rgba_stride};
            if (scaled) h_scaletab[k] = ScaleSrc{(unsigned long long)(uintptr_t)it.scale_src, (uint32_t)(rgba ? 4 * h->sw : h->sw),
                                                 (uint32_t)(rgba ? 0 : h->fmt == MI355X_H264_INPUT_NV12 ? h->sw : h->sw / 2), (uint32_t)h->fmt, 0};
            if (it.staged && hipStreamWaitEvent(Y.st, it.copied, 0) != hipSuccess) rc = MI355X_H264_E_HIP;
            if (it.staged && it.patch_tiles) {   // the picture came as damage tiles: they go into the slot the upload would have filled
                const size_t item = (size_t)pics[k].item;
                uint8_t* const slot = scaled ? h->d_src + item * h->st_src : rgba ? h->d_rgba + item * h->st_rgba : h->d_stage + item * h->st_stage;
                h_patchtab[npatch++] = PatchSrc{(unsigned long long)(uintptr_t)(h->d_patch + item * h->st_src), (unsigned long long)(uintptr_t)slot,
                                                it.patch_tiles, (uint32_t)h->fmt, (uint32_t)h->sw, (uint32_t)h->sh};
                patch_most = std::max(patch_most, it.patch_tiles); patch_sum += it.patch_tiles;
            }
        }
        const size_t tab_bytes = npatch ? HubCtx::TAB_PATCH + (size_t)npatch * sizeof(PatchSrc) : scaled ? HubCtx::TAB_SCALE + (size_t)n * sizeof(ScaleSrc) : rgba ? HubCtx::TAB_RGBA + (size_t)n * sizeof(RgbaSrc) : HubCtx::TAB_ITEM + (size_t)n * sizeof(uint32_t);
        if (hipMemcpyAsync(c.d_tab, c.h_tab, tab_bytes, hipMemcpyHostToDevice, Y.st) != hipSuccess) rc = MI355X_H264_E_HIP;
        const unsigned long long* const d_srctab = (const unsigned long long*)(c.d_tab + HubCtx::TAB_SRC);
        if (rc == MI355X_H264_OK && npatch) {   // one patch launch for the step (k_patch.h), behind the `copied` waits and in front of every reader of a slot
            hipLaunchKernelGGL(k_patch_step, dim3((patch_most + 3) / 4, (unsigned)npatch), dim3(256), 0, Y.st, (const PatchSrc*)(c.d_tab + HubCtx::TAB_PATCH));
            h->patch_launches++; h->patch_tiles += patch_sum;
        }
        if (rc == MI355X_H264_OK && scaled) {   // one scaling launch for the step: every position, all planes (scale_kernels.h)
            const int w = h->cfg.width, hh = h->cfg.height, th = scale_tile_rows(h->sh, hh);
            const ScalePlane PY = scale_plane_make(h->sw, h->sh, w, hh), PC = scale_plane_make(h->sw / 2, h->sh / 2, w / 2, hh / 2);
            const bool nv12 = h->fmt == MI355X_H264_INPUT_NV12;
            const int ntx_y = scale_tiles_x(w, rgba ? 4 : 1), ntx_c = rgba ? 0 : scale_tiles_x(w / 2, nv12 ? 2 : 1);
            hipLaunchKernelGGL(k_scale_to_i420_step, dim3((unsigned)(ntx_y + (nv12 ? 1 : 2) * ntx_c), (unsigned)((hh + th - 1) / th), (unsigned)n), dim3(256), 0, Y.st,
                               (const ScaleSrc*)(c.d_tab + HubCtx::TAB_SCALE), rgba ? (const unsigned long long*)(c.d_tab + HubCtx::TAB_RGBA) : d_srctab, rgba ? 2 : 1,
                               PY, PC, ntx_y, ntx_c, th);
        }
        if (rc == MI355X_H264_OK && rgba) {   // one conversion launch for the step, in front of the first kernel that reads samples
            const int w = h->cfg.width, hh = h->cfg.height;
            launch_rgba_to_i420_step(h->colour.described ? colour_variant(h->colour.matrix, h->colour.full_range) : 0,
                                     dim3((unsigned)((w / 2 + 255) / 256), (unsigned)(hh / 2), (unsigned)n), Y.st,
                                     (const RgbaSrc*)(c.d_tab + HubCtx::TAB_RGBA), d_srctab, w, hh);
        }
        if (rc == MI355X_H264_OK) {
            St.d_src = nullptr; St.src_item_stride = 0; St.idr = idr; St.n = n;
            St.nv12 = h->fmt == MI355X_H264_INPUT_NV12 && !scaled;   // (a scaling hub's staging picture is I420)
            St.items = pics; St.d_itemtab = (const uint32_t*)(c.d_tab + HubCtx::TAB_ITEM); St.d_srctab = d_srctab;
            // entropy coding beside the loop filter shortens a picture's latency; with many streams open the second HIP stream
            // costs more than the overlap brings (64 streams: 10.9 k -> 12.1 k fps on one stream per step)
            St.sync = &Y; St.one_stream = g_streams_open.load(std::memory_order_relaxed) > 40;
            St.slot = &e->slots[0];
            rc = submit_step(e, St);
        }
        if (rc != MI355X_H264_OK) snprintf(errtxt, sizeof(errtxt), "%s", e->err);
    }
    const uint64_t t1 = now_us();
    if (rc == MI355X_H264_OK) {
        if (hipEventSynchronize(Y.done) != hipSuccess) rc = set_err(errtxt, MI355X_H264_E_HIP, "hipEventSynchronize failed");
    } else (void)hipStreamSynchronize(Y.st);
    if (rc == MI355X_H264_OK) rc = handoff_timeout(Y, errtxt);
    const uint64_t t2 = now_us();
    std::lock_guard<std::mutex> lk(h->launch_mu);   // (finish_item touches the engine's statistics and error text)
    for (int k = 0; k < n; k++) {
        HubItem& it = h->items[pics[k].item];
        it.rc = rc;
        if (rc == MI355X_H264_OK) {
            it.rc = finish_item(e, e->slots[0], St.lay, pics[k], &it.out, &it.out_len, &it.frame_type);
            if (it.rc != MI355X_H264_OK) snprintf(it.err, sizeof(it.err), "%s", e->err);
        } else snprintf(it.err, sizeof(it.err), "%s", errtxt);
        T.rc[k] = it.rc;
    }
    h->us_launch += t1 - t0; h->us_gpu += t2 - t1; h->us_finish += now_us() - t2;
}

}  // namespace

struct mi355x_h264_stream { Hub* hub; int item; };

namespace {

// a damage call's request: rects[0 .. n - 1], or n == MI355X_H264_DAMAGE_DETECT with null rects
struct DamageReq { const mi355x_h264_rect* rects; int n; };
static_assert(sizeof(mi355x_h264_rect) == sizeof(damage::Rect), "the ABI's rectangle is damage.h's");

// dmg: null for the ordinary calls, which transfer the whole picture
int hub_encode(mi355x_h264_stream* s, const HostPicture& in, uint8_t** out, uint32_t* out_len, int* frame_type, const DamageReq* dmg = nullptr)
{
    Hub* h = s->hub;
    HubItem& it = h->items[s->item];
    const int w = h->sw, hh = h->sh, item = s->item;   // the size of the pictures the calls take: the source size of a scaling hub
    const bool rgba = h->fmt == MI355X_H264_INPUT_RGBA;
    // whatever is refused is refused here, on the host, before anything is queued or launched; the stream stays usable
    auto refuse = [&](const char* why) { return set_err(it.err, MI355X_H264_E_ARG, "%s", why); };
    if (in.layout != HUB_IN_DEVICE && in.layout != h->fmt) return refuse("the host picture's layout is not the one the stream was opened with");
    if (in.layout == PIC_I420 && (in.stride[0] < w || in.stride[1] < w / 2 || in.stride[2] < w / 2)) return refuse("stride smaller than width");
    if (in.layout == PIC_NV12 && (in.stride[0] < w || in.stride[1] < w)) return refuse("stride smaller than width");
    if (in.layout == PIC_RGBA && in.stride[0] < 4 * w) return refuse("stride smaller than 4 * width");
    if (in.layout == HUB_IN_DEVICE && rgba && ((uintptr_t)in.p[0] & 7) != 0) return refuse("RGBA picture not aligned to 8 bytes");
    const bool detect = dmg && dmg->n == MI355X_H264_DAMAGE_DETECT;
    if (dmg && detect && dmg->rects) return refuse("damage: MI355X_H264_DAMAGE_DETECT takes no rectangles");
    if (dmg && !detect) {
        it.mark.clear();
        if (!damage::rects_to_tiles(w, hh, (const damage::Rect*)dmg->rects, dmg->n, it.mark))
            return refuse("damage: a negative count, a count without rectangles, or a rectangle of negative width or height");
    }
    if (hipSetDevice(h->cfg.device) != hipSuccess) return set_err(it.err, MI355X_H264_E_HIP, "hipSetDevice");
    const uint64_t t_in = now_us();
    const bool staged = in.layout != HUB_IN_DEVICE;
    bool ok = true;
    it.patch_tiles = 0;
    it.up_bytes = staged ? picture_bytes(in.layout, w, hh) : 0; it.up_tiles = staged ? (uint32_t)damage::tiles_total(w, hh) : 0;
    it.up_mode = staged ? damage::MODE_WHOLE : damage::MODE_IN_PLACE;
    // the payload pair comes with the hub's first damage call, valid slot or not (under the scheduler's lock, as the other pairs)
    auto patch_pair = [&] { return !dmg || DM_PAIR(h->mem, h->d_patch, h->h_patch, h->st_src * h->sched.cap); };
    if (staged && dmg && it.slot_valid) {
        // 0. a damage call on a valid slot: the slot and its pinned twin hold the stream's last picture (the stream's calls are
        // synchronous: every reader of the slot finished before the last call returned).  The damaged tiles go into the twin, which
        // then holds the picture that is encoded; over the link goes the payload (damage.h) for the step's patch launch, or the
        // twin whole when the payload would not be smaller, or nothing.
        const int nopen = h->sched.begin_upload(patch_pair);
        if (nopen < 0) return set_err(it.err, MI355X_H264_E_NOMEM, "no memory for the damage payloads");
        const size_t st = h->scaled ? h->st_src : rgba ? h->st_rgba : h->st_stage, off = (size_t)item * st;
        uint8_t* const hs = (h->scaled ? h->h_src : rgba ? h->h_rgba : h->h_stage) + off, * const ds = (h->scaled ? h->d_src : rgba ? h->d_rgba : h->d_stage) + off;
        hipStream_t cs = h->copy_st[item % Hub::NCOPY];
        const damage::Picture pic{in.layout, {in.p[0], in.p[1], in.p[2]}, {in.stride[0], in.stride[1], in.stride[2]}};
        if (detect) damage::detect_and_copy(pic, w, hh, hs, it.mark);
        else damage::copy_tiles(pic, w, hh, it.mark, hs);
        const size_t ntiles = damage::count_tiles(it.mark);
        it.d_in = nullptr;
        if (h->scaled) it.scale_src = ds;
        else if (rgba) { it.rgba_src = ds; it.rgba_stride = (size_t)w * 4; }
        it.up_tiles = (uint32_t)ntiles; it.up_mode = damage::upload_mode(in.layout, w, hh, ntiles);
        if (it.up_mode == damage::MODE_PATCHED) {
            uint8_t* const hp = h->h_patch + (size_t)item * h->st_src;
            it.up_bytes = damage::pack_payload(in.layout, w, hh, hs, it.mark, hp);
            it.patch_tiles = (uint32_t)ntiles;
            ok = hipMemcpyAsync(h->d_patch + (size_t)item * h->st_src, hp, it.up_bytes, hipMemcpyHostToDevice, cs) == hipSuccess && hipEventRecord(it.copied, cs) == hipSuccess;
        } else if (it.up_mode == damage::MODE_WHOLE) {
            ok = hipMemcpyAsync(ds, hs, it.up_bytes, hipMemcpyHostToDevice, cs) == hipSuccess && hipEventRecord(it.copied, cs) == hipSuccess;
        } else it.up_bytes = 0;   // nothing changed: no transfer, no patch; the step waits for the slot's last transfer, long arrived
    } else if (staged && h->scaled) {
        // a scaling hub's host picture goes to the stream's source staging slot, which comes with the hub's first host picture; the
        // step's scaler reads it after it.copied
        const int nopen = h->sched.begin_upload([&] { return DM_PAIR(h->mem, h->d_src, h->h_src, h->st_src * h->sched.cap) && patch_pair(); });
        if (nopen < 0) return set_err(it.err, MI355X_H264_E_NOMEM, "no memory for the source staging pictures");
        const size_t off = (size_t)item * h->st_src;
        it.d_in = nullptr; it.scale_src = h->d_src + off;
        ok = stage_picture(in, w, hh, h->h_src + off, h->d_src + off, h->copy_st[item % Hub::NCOPY], in.layout == PIC_I420 && nopen <= 4 ? 4 : 1) == hipSuccess &&
             hipEventRecord(it.copied, h->copy_st[item % Hub::NCOPY]) == hipSuccess;
    } else if (h->scaled) {
        it.d_in = nullptr; it.scale_src = in.p[0];   // read where it lies by the step's scaler, during the call
    } else if (staged) {
        // 1. a host picture goes to the stream's staging slot (RGBA: to its RGBA staging slot, which comes with the hub's first host
        // RGBA picture; the step's conversion launch writes the I420 slot): pinned copy, then the transfer on the item's copy
        // stream; it.copied says when it has arrived
        const int nopen = h->sched.begin_upload([&] { return (in.layout != PIC_RGBA || DM_PAIR(h->mem, h->d_rgba, h->h_rgba, h->st_rgba * h->sched.cap)) && patch_pair(); });
        if (nopen < 0) return set_err(it.err, MI355X_H264_E_NOMEM, "no memory for the RGBA staging pictures");
        const size_t off = (size_t)item * (in.layout == PIC_RGBA ? h->st_rgba : h->st_stage);
        uint8_t* const hs = (in.layout == PIC_RGBA ? h->h_rgba : h->h_stage) + off, * const ds = (in.layout == PIC_RGBA ? h->d_rgba : h->d_stage) + off;
        hipStream_t cs = h->copy_st[item % Hub::NCOPY];
        // few streams: four pieces, so that the copy of piece k + 1 runs while piece k is on the bus (latency); many streams: one
        // transfer per picture (every queued command costs, and other streams' transfers fill the bus anyway: 16 / 32 / 64 streams
        // went from 7.3 / 8.0 / 8.6 k to 8.8 / 11.5 / 10.9 k fps with this alone, profiles/r03_hub_sweep_*.log)
        const int pieces = in.layout == PIC_I420 && nopen <= 4 ? 4 : 1;
        it.d_in = nullptr;
        if (in.layout == PIC_RGBA) { it.rgba_src = ds; it.rgba_stride = (size_t)w * 4; }
        ok = stage_picture(in, w, hh, hs, ds, cs, pieces) == hipSuccess && hipEventRecord(it.copied, cs) == hipSuccess;
    } else if (rgba) {
        // a device picture is read where it lies: nothing is copied and nothing waited for.  RGBA: by the step's conversion launch,
        // which writes the item's I420 staging slot; I420 / NV12: by the encoder kernels themselves
        it.d_in = nullptr; it.rgba_src = in.p[0]; it.rgba_stride = (size_t)w * 4;
    } else it.d_in = in.p[0];
    it.staged = staged;
    const uint64_t t_q = now_us();
    // 2. queue the picture; lead a step or wait for the one that takes it
    h->us_upload += t_q - t_in;
    if (!h->sched.encode(item, staged, ok, [&](HubStep& T) { hub_run_step(h, T); })) { it.slot_valid = false; return set_err(it.err, MI355X_H264_E_HIP, "upload of the picture failed"); }
    it.slot_valid = staged && it.rc == MI355X_H264_OK;
    h->us_total += now_us() - t_in;
    *out = it.out; *out_len = it.out_len;
    if (frame_type) *frame_type = it.frame_type;
    return it.rc;
}

}  // namespace
