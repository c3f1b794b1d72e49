// media_amd/csrc/pic_store.h -- the picture store: what reconstruction, the intra row wavefront and the loop filter need, whoever
// drives them.  It is the part of the device memory that the encoder engine (engine.h, which IS a store plus what coding a stream
// takes) and the decoder groups (dec_group.h, which own a store and nothing of the encoder's) share: the reconstruction ring, the
// per-macroblock arrays the kernels hand each other, the hand-off granules of the row wavefronts, the per-picture flags and the two
// serial counters.  With it: what a step in flight is launched on and waited for with (StepSync), the check of the ring's zeroed
// slack for the guard mode of the owner's list of allocations (DevMem, dev_mem.h), and the parameter blocks of the kernels as far as they come from a store alone.  A store owns no stream.  Part of the
// one translation unit mi355x_h264.hip, which includes the kernels before this file.
#pragma once

#define HIPCHK(err, call)                                                                                    \
    do {                                                                                                     \
        hipError_t _r = (call);                                                                              \
        if (_r != hipSuccess) return set_err((err), MI355X_H264_E_HIP, "%s: %s", #call, hipGetErrorString(_r)); \
    } while (0)
// for the set-up functions that hand the hipError_t on (their callers undo and translate): t_failed_call (dev_mem.h) names the call
#define HIPTRY(call)                                                     \
    do {                                                                  \
        hipError_t _r = (call);                                           \
        if (_r != hipSuccess) { t_failed_call = #call; return _r; }       \
    } while (0)

namespace {

// What one step in flight needs to be launched and waited for: its stream pair (entropy coding forks to ec), the fork /
// join events, the event behind its last command and the wavefront kernels' time-out flag (pinned).  An engine slot, a hub
// context and a decoder group each hold one.
struct StepSync {
    hipStream_t st = nullptr, ec = nullptr;
    hipEvent_t recon_ready = nullptr, entropy_done = nullptr, done = nullptr;
    unsigned* h_err = nullptr;
    bool own_streams = false;
};
// st == nullptr: a stream pair of its own (one stream for both when one_stream); else the caller's pair
hipError_t sync_create(StepSync& y, hipStream_t st, hipStream_t ec, bool one_stream)
{
    if (!st) {
        y.own_streams = true;
        HIPTRY(hipStreamCreateWithFlags(&y.st, hipStreamNonBlocking));
        if (one_stream) y.ec = y.st;
        else HIPTRY(hipStreamCreateWithFlags(&y.ec, hipStreamNonBlocking));
    } else { y.st = st; y.ec = ec; }
    for (hipEvent_t* ev : {&y.done, &y.recon_ready, &y.entropy_done}) HIPTRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    HIPTRY(hipHostMalloc((void**)&y.h_err, sizeof(unsigned), hipHostMallocDefault));
    *y.h_err = 0;
    return hipSuccess;
}
void sync_destroy(StepSync& y)
{
    if (y.own_streams && y.st) {
        (void)hipStreamSynchronize(y.st);
        if (y.ec && y.ec != y.st) { (void)hipStreamSynchronize(y.ec); (void)hipStreamDestroy(y.ec); }
        (void)hipStreamDestroy(y.st);
    }
    for (hipEvent_t ev : {y.done, y.recon_ready, y.entropy_done}) if (ev) (void)hipEventDestroy(ev);
    if (y.h_err) (void)hipHostFree(y.h_err);
    y = StepSync();
}
// the wavefront kernels' time-out flag of a finished step: read, cleared (it is per report) and put into words
int handoff_timeout(StepSync& y, char (&err)[256])
{
    const unsigned flag = *y.h_err;
    if (!flag) return MI355X_H264_OK;
    *y.h_err = 0;
    return set_err(err, MI355X_H264_E_INTERNAL, "wavefront kernel hand-off timed out (flag %u)", flag);
}

// HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4): an engine has two streams, a stream hub seven, a decoder
// group one, and a host process runs several.  Ask for more before the runtime comes up - unless the host has chosen (measured: 64
// plugin streams 7.4 k fps on 4 queues, 10.4 k on 32).  Has no effect once another HIP user has initialised the runtime.
void ask_for_hw_queues()
{
    static std::once_flag once;
    std::call_once(once, [] { setenv("GPU_MAX_HW_QUEUES", "16", 0); });
}

struct PicStore {
    enum { MAX_BUF = 4 };
    int device = 0;
    int mbw = 0, mbh = 0, cw = 0, ch = 0, nmb = 0;
    int G = 1;                               // items: the pictures of a lockstep step (closed GOPs, streams) each have their own of everything
    int nbuf = 2;                            // ring slots per item
    size_t st_y = 0, st_c = 0, st_handoff = 0;  // per-item strides
    uint8_t* d_planes[MAX_BUF][3] = {{nullptr}};  // item 0's ring: [slot][plane]
    // the planes lie [item][ring slot]: d_planes[b][p] = d_plane_base[p] + b * st_ring, st_y / st_c (the item strides) = nbuf
    // ring strides - so that a launch that takes its positions from a table can address every item's OWN ring slot from one base pointer
    uint8_t* d_plane_base[3] = {nullptr, nullptr, nullptr};
    size_t st_ring_y = 0, st_ring_c = 0;
    MbInfo* d_mb = nullptr;
    int16_t* d_levels = nullptr;
    uint8_t* d_aux = nullptr;                // [G][nmb][16] Intra4x4 modes
    int16_t* d_mvq = nullptr;                // [G][nmb][8] vectors of the four 8x8 quadrants of inter macroblocks
    unsigned* d_anybs = nullptr;             // [G] picture serial when any boundary strength is non-zero
    unsigned* d_anypcm = nullptr;            // [G] == pic_serial: the picture holds an I_PCM macroblock (not loop-filtered)
    unsigned* d_anyintra = nullptr;          // [G] == pic_serial: P picture with macroblocks for the intra pass
    unsigned* d_stepintra = nullptr;         // one word == pic_serial: some P picture of the step has macroblocks for the intra pass
    unsigned long long* d_handoff = nullptr; // row-to-row hand-off of the wavefront kernels
    uint32_t* d_bs = nullptr;                // boundary strengths, 32 B per macroblock
    unsigned serial = 0;                     // of the wavefront launches
    unsigned pic_serial = 0;                 // changes every picture, never 0
    DevMem mem;                              // every hipMalloc / hipHostMalloc of the store - and of an engine built on it
    bool made() const { return d_plane_base[0] != nullptr; }
};

// the arrays of `items` pictures of mbw x mbh macroblocks with `nbuf` ring slots each, zeroed where the kernels count on it.  The
// consumers run on non-blocking streams, which do not wait for the zeroing: hence the synchronize.  On failure the caller destroys.
hipError_t pic_store_create(PicStore& s, int device, int mbw, int mbh, int items, int nbuf)
{
    ask_for_hw_queues();
    DevMem& M = s.mem;
    HIPTRY(hipSetDevice(device));
    s.device = device; s.mbw = mbw; s.mbh = mbh; s.cw = 16 * mbw; s.ch = 16 * mbh; s.nmb = mbw * mbh; s.G = items; s.nbuf = nbuf;
    const size_t ysz = (size_t)s.cw * s.ch;
    const size_t Gn = (size_t)items, nmb = Gn * s.nmb;   // (nmb: macroblocks of all items)
    s.st_ring_y = ysz + 256; s.st_ring_c = ysz / 4 + 256;
    s.st_y = s.st_ring_y * nbuf; s.st_c = s.st_ring_c * nbuf;
    static const char* const plane_name[3] = {"d_plane_base[0]", "d_plane_base[1]", "d_plane_base[2]"};
    for (int p = 0; p < 3; p++) {
        HIPTRY(M.dev(&s.d_plane_base[p], (p ? s.st_c : s.st_y) * Gn, true, plane_name[p]));
        for (int b = 0; b < nbuf; b++) s.d_planes[b][p] = s.d_plane_base[p] + (size_t)b * (p ? s.st_ring_c : s.st_ring_y);
    }
    HIPTRY(M.dev(&s.d_mb, nmb * sizeof(MbInfo), true, "d_mb"));
    HIPTRY(M.dev(&s.d_levels, nmb * LV_STRIDE * sizeof(int16_t), false, "d_levels"));
    HIPTRY(M.dev(&s.d_mvq, nmb * 8 * sizeof(int16_t), true, "d_mvq"));
    HIPTRY(M.dev(&s.d_aux, nmb * 16, true, "d_aux"));
    HIPTRY(M.dev(&s.d_anybs, Gn * sizeof(unsigned), true, "d_anybs"));
    HIPTRY(M.dev(&s.d_anypcm, Gn * sizeof(unsigned), true, "d_anypcm"));
    HIPTRY(M.dev(&s.d_anyintra, Gn * sizeof(unsigned), true, "d_anyintra"));
    HIPTRY(M.dev(&s.d_stepintra, sizeof(unsigned), true, "d_stepintra"));
    s.st_handoff = (size_t)s.nmb * 24;
    HIPTRY(M.dev(&s.d_handoff, Gn * s.st_handoff * sizeof(unsigned long long), true, "d_handoff"));
    HIPTRY(M.dev(&s.d_bs, nmb * 32, false, "d_bs"));
    HIPTRY(hipDeviceSynchronize());
    return hipSuccess;
}
// nothing of the owner's may be in flight.  The store's guard setting (dev_mem.h) stays: it is the owner's, taken at its creation
void pic_store_destroy(PicStore& s)
{
    s.mem.free_all();
    const size_t guard = s.mem.guard;
    const bool poison = s.mem.poison;
    s = PicStore();
    s.mem.guard = guard; s.mem.poison = poison;
}

// The 256 bytes behind every ring slot of every item are zeroed at creation and no kernel stores there: inner guards that cost
// nothing.  With the guard mode on, the check looks at them too: one region per plane, item and slot, reported under the name
// "ring slack <plane>" with offsets from the plane's first byte.  Returns the damaged regions, -1 when a copy failed
int store_check_slack(const PicStore& s, std::vector<MemDamage>& found, int* regions)
{
    if (!s.mem.guard || !s.made()) return 0;
    static const char* const name[3] = {"ring slack d_plane_base[0]", "ring slack d_plane_base[1]", "ring slack d_plane_base[2]"};
    const size_t before = found.size(), slots = (size_t)s.G * s.nbuf;
    std::vector<uint8_t> tmp(slots * 256);
    for (int p = 0; p < 3; p++) {
        const size_t st = p ? s.st_ring_c : s.st_ring_y, used = st - 256;
        if (hipMemcpy2D(tmp.data(), 256, s.d_plane_base[p] + used, st, 256, slots, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (size_t k = 0; k < slots; k++) {
            MemDamage d{name[p], true, 0, 0, 0};
            for (size_t i = 0; i < 256; i++)
                if (tmp[k * 256 + i]) {
                    const long long off = (long long)(k * st + used + i);
                    if (!d.count) d.first = off;
                    d.last = off; d.count++;
                }
            if (d.count) found.push_back(d);
        }
        if (regions) *regions += (int)slots;
    }
    return (int)(found.size() - before);
}

// ---- the parameter blocks of the kernels, as far as they come from the store alone (the engine's frame_params and submit_step and
// the decoder groups' dg_step add what is theirs) ----
inline unsigned next_nonzero(unsigned& serial) { serial = serial == 0xFFFFFFFFu ? 1u : serial + 1u; return serial; }   // changes every time, never 0

FrameParams store_frame_params(PicStore* s)   // takes the next picture serial
{
    FrameParams P{};
    P.cw = s->cw; P.ch = s->ch; P.mbw = s->mbw; P.mbh = s->mbh;
    P.mb = s->d_mb; P.levels = s->d_levels; P.mvq = s->d_mvq; P.aux = s->d_aux;
    P.st_y = s->st_y; P.st_c = s->st_c; P.st_mb = s->nmb;
    P.mbdiv.inv = recip32(s->mbw);
    P.anypcm = s->d_anypcm; P.anyintra = s->d_anyintra; P.stepintra = s->d_stepintra; P.pic_serial = next_nonzero(s->pic_serial);
    return P;
}
IntraRowParams intra_row_params(PicStore* s, const FrameParams& P, unsigned* h_err, int npic)   // takes the next wavefront serial
{
    IntraRowParams R{};
    R.p = P; R.handoff = s->d_handoff; R.st_handoff = s->st_handoff; R.err = h_err;
    R.serial = next_nonzero(s->serial);
    R.npic = npic;
    return R;
}
// pl: the planes being filtered (or their base: launches by table); qp: the picture's (thresholds of every edge unless the launch reads mbqp)
DbParams db_params(const PicStore* s, uint8_t* const pl[3], const SliceRows& sl, int qp)
{
    DbParams D{};
    for (int p = 0; p < 3; p++) D.pl[p] = pl[p];
    D.mb = s->d_mb; D.cw = s->cw; D.ch = s->ch; D.mbw = s->mbw; D.mbh = s->mbh; D.sl = sl; D.bs = (const uint8_t*)s->d_bs;
    fill_filter_thresholds(D, qp);
    return D;
}
DbRowParams db_row_params(const PicStore* s, const DbParams& D, unsigned* h_err, unsigned serial, unsigned pic_serial, int row0, int npic)
{
    DbRowParams R{};
    R.d = D; R.handoff = s->d_handoff; R.err = h_err;
    R.st_y = s->st_y; R.st_c = s->st_c; R.st_handoff = s->st_handoff; R.st_mb = s->nmb;
    R.serial = serial; R.row0 = row0;
    R.bs = s->d_bs; R.anybs = s->d_anybs;
    R.anypcm = s->d_anypcm; R.anyintra = s->d_anyintra; R.pic_serial = pic_serial;
    R.npic = npic;
    return R;
}

}  // namespace
