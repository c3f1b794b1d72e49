// media_amd/csrc/dec_group.h -- decoder groups (include/mi355x_h264_dec.h, mi355x_h264_dec_group_*): the next pictures of up to 64
// streams reconstructed in ONE lockstep step in one picture store (pic_store.h) with one item per stream, as the stream hub does
// for encoders in its engine's.  A group owns that store, one stream and nothing of the encoder's.  A step is
// one set of uploads and one set of launches whatever the number of streams: the streams' access units are parsed side by side on
// a small pool of threads (dec_group_sched.h, which also rotates the two sets of pinned buffers), every parsed picture is copied
// into its item's slice of group-wide pinned arrays laid [item][...], and each array then travels in one transfer that covers the
// items from the lowest to the highest taking part (a stream that sits the step out inside that range has its stale slice sent
// along: the per-macroblock arrays on the device are scratch of the step, nobody reads an absent item's).  What the pictures of a
// step have of their own - ring slots, reference lists, offsets, filter controls, slice bands - is the step's position table
// (dev_common.h DecPos); the kernels are k_dec_widen_pos / _inter_pos / _bs_pos, k_dec_resid, k_pintra_rows<true, true> and
// k_deblock_rows<BS4, true, true>.  This is the project's ONE decoder: the decoder peer (decoder.h) is a group of one stream.  What
// the general form costs such a group is the copy of the parsed picture into the pinned set, about 4.5 MB per 1080p picture; the
// parse job makes it (a parser that writes into the set in place is the follow-up).
#pragma once
#include "dec_group_sched.h"
#include "dec_out.h"

namespace {

struct DecGroupStream {
    h264dec::Parser parser;
    int have_refs = 0, max_refs = 1;
    int cur = 0;         // ring slot its next picture is written to
    int last = -1;       // ring slot of its last decoded picture
    int width = 0, height = 0, crop_x = 0, crop_y = 0;
    uint64_t pictures = 0;
    int64_t last_serial = 0;   // serial number of the step that decoded its last picture
    h264dec::Vui vui;    // of the sequence parameter set its last decoded picture was coded under (mi355x_h264_dec_colour)
    int rgba_override = -1;   // mi355x_h264_dec_set_rgba_colour: the variant RGBA output applies whatever the stream says; -1: follow the stream
    int out_w = 0, out_h = 0; // mi355x_h264_dec_group_set_output_size: the size its pictures are delivered at; 0, 0: their own
    // loss mode (include/mi355x_h264_dec.h, "loss mode"; the arithmetic: dec_loss.h).  0: strict, nothing below is touched but `since`
    // - unless the stream HAS concealed (taint is not empty): the maps then go on in strict mode too, until the geometry goes
    int loss = 0;
    bool virt = false;        // its reference pictures are the ring slots of `refs` (a gap or a join since the last IDR picture);
                              // false: the ring's plain rotation, age a in slot cur - 1 - a
    dec_loss::RefSlots refs;
    std::vector<uint8_t> taint;   // [ring slot][macroblock]: the damage maps, made with the first picture decoded in conceal mode
    int tainted = 0, concealed = 0, gap = 0, recovery = -1;   // of its last picture (mi355x_h264_dec_damage out[0..3])
    int64_t since = 0;        // pictures decoded since its last loss, join or refusal
    bool joined = false;      // joined without an IDR picture and not clean since
    // the step in hand
    const uint8_t* au = nullptr;
    size_t len = 0;
    int prc = 0;         // what the parser said: 1 picture, 0 none, -1 refused, -2 out of memory
    bool copied = false; // its picture lies in the pinned set
    char err[256] = {0};
};

// the per-macroblock arrays of a step: bytes per macroblock, and the arrays themselves (pinned: one per set; device: one)
enum { DG_MB, DG_MVQ, DG_AUX, DG_LV8, DG_QP, DG_AVAIL, DG_MV4, DG_REFQ, DG_ARRAYS };
constexpr size_t DG_BYTES[DG_ARRAYS] = {sizeof(MbInfo), 16, 16, LV_STRIDE, 1, 1, 64, 4};

}  // namespace

struct mi355x_h264_dec_group {
    int device = 0, nstreams = 0;
    bool resize = false;                 // an IDR picture of another coded size re-makes the geometry.  Honoured for a group of ONE
                                         // stream only (a step of several has rows and copies in the arrays that would go); the
                                         // decoder peer sets it: not in the public ABI, where a group keeps its first size
    PicStore store;                      // made for the group's geometry (that of the first IDR picture it meets): store.made()
    StepSync sync;                       // the group's one stream; its h_err is the wavefront time-out flag
    DecGroupStream* st = nullptr;        // [nstreams]
    DecGroupSched sched;
    uint8_t* h_arr[2][DG_ARRAYS] = {};   // pinned sets, [item][macroblock]
    uint8_t* d_arr[DG_ARRAYS] = {};      // device (MbInfo, quadrant vectors and Intra4x4 modes are the store's own arrays)
    DecPos* h_tab[2] = {nullptr, nullptr};
    DecPos* d_tab = nullptr;
    DecBigLevel* h_big[2] = {nullptr, nullptr};
    size_t h_big_cap[2] = {0, 0};
    DecBigLevel* d_big = nullptr;
    size_t d_big_cap = 0;
    DevMem mem;
    hipEvent_t up_done[2] = {nullptr, nullptr};
    bool busy = false;                   // a step is in flight on the group's stream
    int flight[DEC_GROUP_MAX_STREAMS];   // its streams
    int nflight = 0;
    int intra_slots = 32, filter_slots = 32;   // pictures the row wavefronts hold at a time (the rest are walked to)
    int64_t step_serial = 0, last[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (last_step's out[11] / out[12] are the DevMem totals)
    double last_ms[2] = {0, 0};          // the last step's parse and launch time, untruncated (last[5] / last[6] are whole microseconds)
    // output (k_dec_out.h, k_dec_out_scale.h).  rd: read_all's table and staging; its device staging buffer also serves the armed steps (everything
    // is ordered on the group's stream).  Armed: the step's table of output positions lies behind its DecPos rows in tables of
    // their own (h_tabx / d_tabx: DecPos [streams], then DecOutPos or - a stream has an output size - DecOutScalePos [streams]), so that
    // one transfer carries both.
    struct Out {
        DecOutBuf rd;
        bool armed = false, ready = false;
        int layout = 0, row_align = 1;
        uint8_t* h_tabx[2] = {nullptr, nullptr};
        uint8_t* d_tabx = nullptr;
        uint8_t* h_set[2] = {nullptr, nullptr};   // the two pinned output sets
        size_t set_cap = 0;
        hipEvent_t done[2] = {nullptr, nullptr};  // the copy into the set has finished
        mi355x_h264_dec_out_pic pics[2][DEC_GROUP_MAX_STREAMS];
        int cur = 0, count = 0;                   // the set of the last armed step; armed steps so far (0, 1, 2 = two or more)
    } out;
    char err[256] = {0};
};

namespace {

int env_int(const char* name, int lo, int hi, int dflt)
{
    const char* v = getenv(name);
    if (!v || !*v) return dflt;
    return std::min(hi, std::max(lo, atoi(v)));
}

void dg_drop_refs(DecGroupStream& s) { s.have_refs = 0; s.since = 0; s.parser.lose_refs(); }

// RefPicList0 entry r of the picture in hand as a ring slot, and whether that entry is a stand-in picture (dec_loss.h)
int dg_ref_age(const DecGroupStream& s, const h264dec::Picture& pic, int r)
{
    return std::min(r < pic.num_ref_active ? pic.ref_age[r] : r, std::max(0, s.have_refs - 1));
}
int dg_ref_slot(const DecGroupStream& s, const h264dec::Picture& pic, int r, int nbuf)
{
    const int age = dg_ref_age(s, pic, r);
    return s.virt ? s.refs.slot[age] : (s.cur + nbuf - 1 - age) % nbuf;
}

// the damage map of the picture in hand into the slot it is written to, and the stream's report (conceal mode only)
void dg_damage(DecGroupStream& s, const h264dec::Picture& pic, int nbuf)
{
    const size_t nmb = (size_t)pic.mbw * pic.mbh;
    if (s.taint.size() != nmb * nbuf) s.taint.assign(nmb * nbuf, 0);
    dec_loss::TaintPic t;
    t.mbw = pic.mbw; t.mbh = pic.mbh;
    t.type = &pic.mb[0].type; t.type_stride = sizeof(h264dec::MbRec);
    t.mv4 = pic.mv4.data(); t.refq = pic.refq.data(); t.avail = pic.mbavail.data();
    t.concealed = pic.concealed.empty() ? nullptr : pic.concealed.data();
    t.deblock_idc = pic.deblock_idc;
    for (int r = 0; r < 3; r++) {
        const bool standin = s.have_refs < 1 || (s.virt && s.refs.standin[dg_ref_age(s, pic, r)]);
        t.ref[r] = standin ? nullptr : s.taint.data() + (size_t)dg_ref_slot(s, pic, r, nbuf) * nmb;
    }
    s.tainted = dec_loss::taint_picture(t, s.taint.data() + (size_t)s.cur * nmb, &s.concealed);
    s.gap = pic.gap;
    if (pic.joined) s.joined = true;
    if (s.tainted == 0) s.joined = false;
    if (pic.joined || pic.gap > 0 || s.concealed > 0) s.since = -1;   // (the picture of a loss counts 0: dg_step adds one)
}

// The variant of the RGBA conversion a stream's pictures get (k_dec_out.h, DecOutPos.colour): the override if there is one, else
// what the stream describes when its matrix_coefficients are 1 (BT.709), 5 or 6 (both have the BT.601 numbers); every other
// stream, one without a description included, is BT.601 limited as before there were descriptions
int dg_rgba_variant(const DecGroupStream& s)
{
    if (s.rgba_override >= 0) return s.rgba_override;
    const h264dec::Vui& v = s.vui;
    if (!v.present || !v.colour || (v.matrix != 1 && v.matrix != 5 && v.matrix != 6)) return 0;
    return (v.matrix == 1 ? 1 : 0) | (v.full_range ? 2 : 0);
}
int dg_out_variant(const DecGroupStream& s, int layout) { return layout == DEC_OUT_RGBA ? dg_rgba_variant(s) : -1; }

// The size stream s's last picture is delivered at: its own, or the output size set.  false: the picture cannot be resampled to
// that size; the stream's report says so with both sizes, and the call delivers the other streams
bool dg_out_size(DecGroupStream& s, int& W, int& H)
{
    W = s.out_w ? s.out_w : s.width; H = s.out_w ? s.out_h : s.height;
    if (!s.out_w || out_size_serves(s.width, s.height, W, H)) return true;
    snprintf(s.err, sizeof(s.err), "output size %dx%d cannot be made from a picture of %dx%d: W <= w <= 4 W and H <= h <= 4 H must hold", W, H, s.width, s.height);
    return false;
}
// one more row of a call's table: stream i's picture in ring slot `slot`, delivered at W x H at byte `off`
void dg_out_row(OutCall& c, const DecGroupStream& s, int i, int slot, int W, int H, const OutGeom& geo, size_t off, int layout)
{
    c.rows[c.n] = DecOutPos{(uint32_t)i, (uint32_t)slot, (uint32_t)s.crop_x, (uint32_t)s.crop_y, (uint32_t)W, (uint32_t)H,
                            (uint32_t)geo.stride, (uint32_t)geo.cstride, (unsigned long long)off, (uint32_t)std::max(0, dg_out_variant(s, layout)), 0u};
    c.src[c.n][0] = s.width; c.src[c.n][1] = s.height;
    c.scaled |= s.out_w != 0;
    c.n++;
}

// the step in flight has finished; a wavefront that timed out leaves none of the step's pictures usable as a reference
int dg_wait(mi355x_h264_dec_group* g)
{
    if (!g->busy) return MI355X_H264_OK;
    g->busy = false;
    HIPCHK(g->err, hipStreamSynchronize(g->sync.st));
    const int rc = handoff_timeout(g->sync, g->err);
    if (rc) for (int k = 0; k < g->nflight; k++) dg_drop_refs(g->st[g->flight[k]]);
    return rc;
}

// store and arrays go (nothing in flight); the group's stream and events stay
void dg_free_geometry(mi355x_h264_dec_group* g)
{
    pic_store_destroy(g->store);
    g->mem.free_all();
    for (int k = 0; k < 2; k++) {
        for (auto& p : g->h_arr[k]) p = nullptr;
        g->h_tab[k] = nullptr;
        g->h_big[k] = nullptr; g->h_big_cap[k] = 0;
    }
    for (auto& p : g->d_arr) p = nullptr;
    g->d_tab = nullptr;
    g->d_big = nullptr; g->d_big_cap = 0;
    hipEvent_t ev[2] = {g->out.done[0], g->out.done[1]};
    const bool armed = g->out.armed;
    const int layout = g->out.layout, row_align = g->out.row_align;
    g->out = mi355x_h264_dec_group::Out();   // (its buffers were the geometry's: they come again with the next one)
    g->out.done[0] = ev[0]; g->out.done[1] = ev[1]; g->out.armed = armed; g->out.layout = layout; g->out.row_align = row_align;
}

// the buffers of an armed group, for the geometry at hand and the layout armed: sized for every stream's picture at the coded size
int dg_out_prepare(mi355x_h264_dec_group* g)
{
    mi355x_h264_dec_group::Out& o = g->out;
    const size_t S = (size_t)g->nstreams;
    const size_t need = S * out_align(out_geom(o.layout, g->store.cw, g->store.ch, o.row_align).bytes, 256);
    bool ok = true;
    for (int k = 0; k < 2 && ok; k++) {
        if (!o.done[k]) ok = hipEventCreateWithFlags(&o.done[k], hipEventDisableTiming) == hipSuccess;
        if (ok && !o.h_tabx[k]) ok = DM_PINNED(g->mem, o.h_tabx[k], S * (sizeof(DecPos) + sizeof(DecOutScalePos))) == hipSuccess;
    }
    if (ok && !o.d_tabx) ok = DM_DEV(g->mem, o.d_tabx, S * (sizeof(DecPos) + sizeof(DecOutScalePos)), false) == hipSuccess;
    if (ok && need > o.set_cap) {
        for (int k = 0; k < 2; k++) { if (o.h_set[k]) g->mem.drop(o.h_set[k]); o.h_set[k] = nullptr; }
        o.set_cap = 0;
        for (int k = 0; k < 2 && ok; k++) ok = DM_PINNED(g->mem, o.h_set[k], need) == hipSuccess;
        if (ok) o.set_cap = need;
    }
    ok = ok && out_reserve(g->mem, o.rd, need, 0) == hipSuccess;
    if (!ok) return set_err(g->err, MI355X_H264_E_NOMEM, "memory for the output sets of %d streams", g->nstreams);
    o.ready = true;
    return MI355X_H264_OK;
}

// store (four ring slots: the picture being written and three reference pictures) and arrays for the group's geometry
int dg_create_geometry(mi355x_h264_dec_group* g, int mbw, int mbh)
{
    const size_t n = (size_t)mbw * mbh * g->nstreams;
    bool ok = pic_store_create(g->store, g->device, mbw, mbh, g->nstreams, 4) == hipSuccess;
    for (int a = 0; a < DG_ARRAYS && ok; a++) {
        for (int k = 0; k < 2 && ok; k++) ok = DM_PINNED(g->mem, g->h_arr[k][a], n * DG_BYTES[a]) == hipSuccess;
        if (ok && a >= DG_LV8) ok = DM_DEV(g->mem, g->d_arr[a], n * DG_BYTES[a], false) == hipSuccess;
    }
    for (int k = 0; k < 2 && ok; k++) ok = DM_PINNED(g->mem, g->h_tab[k], (size_t)g->nstreams * sizeof(DecPos)) == hipSuccess;
    ok = ok && DM_DEV(g->mem, g->d_tab, (size_t)g->nstreams * sizeof(DecPos), false) == hipSuccess;
    // the lists of large levels at their smallest size, so that the steps of an ordinary stream allocate nothing (dg_step grows them)
    for (int k = 0; k < 2 && ok; k++) if ((ok = DM_PINNED(g->mem, g->h_big[k], 1024 * sizeof(DecBigLevel)) == hipSuccess)) g->h_big_cap[k] = 1024;
    if (ok && (ok = DM_DEV(g->mem, g->d_big, 1024 * sizeof(DecBigLevel), false) == hipSuccess)) g->d_big_cap = 1024;
    if (!ok) {
        dg_free_geometry(g);
        return set_err(g->err, MI355X_H264_E_NOMEM, "memory for the arrays of %d streams of %dx%d macroblocks (%s)", g->nstreams, mbw, mbh, t_failed_call);
    }
    g->d_arr[DG_MB] = (uint8_t*)g->store.d_mb; g->d_arr[DG_MVQ] = (uint8_t*)g->store.d_mvq; g->d_arr[DG_AUX] = g->store.d_aux;
    return MI355X_H264_OK;
}

// `resize`: everything the old coded size owned goes, so that the IDR picture in hand finds the group as a new one does.  Nothing may
// be in flight when the arrays are freed: the step (dg_wait, checked by the caller), whatever else is queued on the group's stream
// - an armed step's copy, the uploads out of BOTH pinned sets -, which the synchronize covers.  No stream keeps a picture.
int dg_drop_geometry(mi355x_h264_dec_group* g)
{
    if (const int wrc = dg_wait(g)) return wrc;
    HIPCHK(g->err, hipStreamSynchronize(g->sync.st));
    g->sched.in_flight[0] = g->sched.in_flight[1] = false;
    dg_free_geometry(g);
    for (int i = 0; i < g->nstreams; i++) { dg_drop_refs(g->st[i]); g->st[i].cur = 0; g->st[i].last = -1; g->st[i].virt = false; g->st[i].taint.clear(); }
    return MI355X_H264_OK;
}

// the parsed picture of stream i into its slice of pinned set k (run by the stream's parse job, or by the caller in the step that
// fixes the geometry)
void dg_copy_picture(mi355x_h264_dec_group* g, int i, int k)
{
    DecGroupStream& s = g->st[i];
    const h264dec::Picture& pic = s.parser.picture();
    const size_t n = (size_t)g->store.nmb;
    static_assert(sizeof(h264dec::MbRec) == sizeof(MbInfo), "layout of the parser's macroblock records");
    const void* src[DG_ARRAYS] = {pic.mb.data(), pic.mvq.data(), pic.aux.data(), pic.levels8.data(), pic.mbqp.data(), pic.mbavail.data(),
                                  pic.mv4.data(), pic.refq.data()};
    for (int a = 0; a < DG_ARRAYS; a++) {
        if (a >= DG_MV4 && !pic.has_inter) continue;   // (not uploaded and not read: no inter macroblock)
        memcpy(g->h_arr[k][a] + (size_t)i * n * DG_BYTES[a], src[a], n * DG_BYTES[a]);
    }
    s.copied = true;
}

int dg_stream_fail(DecGroupStream& s, const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0)
{
    snprintf(s.err, sizeof(s.err), fmt, a, b, c, d);
    dg_drop_refs(s);
    return MI355X_H264_E_STREAM;
}

// one step.  rc[] / got[] per stream; the return value is what concerns the whole group
int dg_step(mi355x_h264_dec_group* g, const uint8_t* const* aus, const size_t* lens, int* got, int* rc)
{
    const int S = g->nstreams;
    g->err[0] = 0;
    for (int i = 0; i < S; i++) { got[i] = 0; rc[i] = MI355X_H264_OK; }
    if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
    int jobs[DEC_GROUP_MAX_STREAMS], njobs = 0;
    for (int i = 0; i < S; i++)
        if (aus[i]) {
            DecGroupStream& s = g->st[i];
            s.au = aus[i]; s.len = lens[i]; s.prc = 0; s.copied = false; s.err[0] = 0;
            jobs[njobs++] = i;
        }
    // the set whose uploads (two steps back) are out of the way; the step in flight reads the other
    hipError_t werr = hipSuccess;
    const int k = g->sched.begin_step([&](int set) { werr = hipEventSynchronize(g->up_done[set]); });
    // (a failure between the first copy out of the set and the event behind the last: the set is handed out again by the next call
    // with no event to wait for, so the copies already queued are waited for here)
    struct EndStep {
        DecGroupSched& s; hipStream_t queued_on = nullptr; bool launched = false;
        ~EndStep() { if (queued_on && !launched) (void)hipStreamSynchronize(queued_on); s.end_step(launched); }
    } end{g->sched};
    if (werr != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipEventSynchronize: %s", hipGetErrorString(werr));
    const double t0 = now_ms();
    const DecGroupSched::ParseFn parse = [g](int i, int set) {
        DecGroupStream& s = g->st[i];
        try {
            s.prc = s.parser.parse_access_unit(s.au, s.len, false);
            if (s.prc > 0 && g->store.made() && s.parser.picture().mbw == g->store.mbw && s.parser.picture().mbh == g->store.mbh) dg_copy_picture(g, i, set);
        } catch (const std::exception&) {
            s.prc = -2;
        }
    };
    g->sched.run(jobs, njobs, k, parse);
    const double t1 = now_ms();
    g->step_serial++;
    g->last[0] = g->step_serial; g->last[1] = g->last[2] = g->last[3] = 0; g->last[4] = g->sched.last_threads;
    g->last_ms[0] = t1 - t0; g->last_ms[1] = 0;
    g->last[5] = (int64_t)((t1 - t0) * 1e3); g->last[6] = 0; g->last[7] = g->last[8] = 0;
    // the step in flight must be out of the way before this one is launched; its time-out flag is looked at here
    if (const int wrc = dg_wait(g)) {
        for (int j = 0; j < njobs; j++) { dg_drop_refs(g->st[jobs[j]]); rc[jobs[j]] = wrc; snprintf(g->st[jobs[j]].err, sizeof(g->st[jobs[j]].err), "%s", g->err); }
        return wrc;
    }
    // which of the parsed pictures this step takes, and the table row of each
    int pos_stream[DEC_GROUP_MAX_STREAMS], npos = 0;
    DecPos* tab = nullptr;
    OutCall ocall;                      // armed: the output positions
    const bool outp = g->out.armed;
    const int oset = g->out.count ? g->out.cur ^ 1 : 0;
    size_t obytes = 0;
    bool any_inter = false, any_intra = false, any_plain = false, any_bs4 = false, any_join = false;
    size_t nbig = 0;
    for (int j = 0; j < njobs; j++) {
        const int i = jobs[j];
        DecGroupStream& s = g->st[i];
        if (s.prc == 0) { if (s.parser.lost()) s.since = 0; continue; }   // (conceal mode: a picture none of whose slices could be used)
        if (s.prc == -2) { snprintf(s.err, sizeof(s.err), "out of host memory while parsing the access unit"); dg_drop_refs(s); rc[i] = MI355X_H264_E_NOMEM; continue; }
        if (s.prc < 0) { snprintf(s.err, sizeof(s.err), "%s", s.parser.error().c_str()); dg_drop_refs(s); rc[i] = MI355X_H264_E_STREAM; continue; }
        const h264dec::Picture& pic = s.parser.picture();
        const h264dec::Sps& sps = s.parser.sps();
        if (S == 1 && g->store.made() && g->resize && pic.idr && (pic.mbw != g->store.mbw || pic.mbh != g->store.mbh)) {
            if (const int drc = dg_drop_geometry(g)) {
                for (int jj = 0; jj < njobs; jj++) dg_drop_refs(g->st[jobs[jj]]);
                return drc;
            }
        }
        if (!g->store.made()) {
            if (!pic.idr && !(s.loss && pic.joined)) { rc[i] = dg_stream_fail(s, "the stream must start with an IDR picture"); continue; }
            if (const int crc = dg_create_geometry(g, pic.mbw, pic.mbh)) {
                for (int jj = 0; jj < njobs; jj++) dg_drop_refs(g->st[jobs[jj]]);
                return crc;
            }
        }
        if (outp && !g->out.ready) {   // (nothing is in flight: dg_wait above)
            if (const int orc = dg_out_prepare(g)) {
                for (int jj = 0; jj < njobs; jj++) dg_drop_refs(g->st[jobs[jj]]);
                return orc;
            }
        }
        const PicStore* const ps = &g->store;
        if (pic.mbw != ps->mbw || pic.mbh != ps->mbh) {
            rc[i] = dg_stream_fail(s, "coded size %dx%d differs from the group's %dx%d", 16 * pic.mbw, 16 * pic.mbh, ps->cw, ps->ch);
            continue;
        }
        if (pic.idr) { s.have_refs = 0; s.virt = false; }
        uint32_t w6 = 0;
        if (s.loss && !pic.idr) {
            const int cap = std::min(std::max(1, sps.max_refs), ps->nbuf - 1);
            if (pic.joined) {
                // a join: every reference picture is ONE grey picture, in the slot behind the one being written (k_dec_ring.h makes it)
                const int grey = (s.cur + ps->nbuf - 1) % ps->nbuf;
                s.refs.join(grey); s.virt = true; s.have_refs = cap;
                w6 = 1u | (1u << (4 + grey));
            } else if (pic.gap > 0 && s.have_refs > 0) {
                // a frame_num gap: the missing pictures are copies of the newest held picture; no step is run for them
                if (!s.virt) { s.refs.from_ring(s.cur, s.have_refs, ps->nbuf); s.virt = true; }
                s.refs.gap(pic.gap);
                s.have_refs = dec_loss::refs_after_gap(s.have_refs, pic.gap, cap);
            }
        }
        if (pic.has_inter && (s.have_refs < 1 || pic.num_ref_active > s.have_refs)) {
            rc[i] = dg_stream_fail(s, "a P picture refers to %d reference pictures, %d are held", pic.num_ref_active, s.have_refs);
            continue;
        }
        bool list_ok = true;
        for (int r = 0; pic.has_inter && r < pic.num_ref_active && r < 3; r++)
            if (pic.ref_age[r] < 0 || pic.ref_age[r] >= s.have_refs) { rc[i] = dg_stream_fail(s, "reference list entry %d is not a held picture", r); list_ok = false; break; }
        if (!list_ok) continue;
        try {
            if (!s.copied) dg_copy_picture(g, i, k);
        } catch (const std::exception&) { rc[i] = MI355X_H264_E_NOMEM; dg_drop_refs(s); continue; }
        s.width = pic.width; s.height = pic.height; s.crop_x = 2 * sps.crop_l; s.crop_y = 2 * sps.crop_t;
        s.max_refs = std::max(1, sps.max_refs);
        s.vui = sps.vui;
        // the table row (dev_common.h DecPos)
        tab = outp ? (DecPos*)g->out.h_tabx[k] : g->h_tab[k];
        DecPos& T = tab[npos];
        memset(&T, 0, sizeof(T));
        const bool filtered = pic.deblock_idc != 1;
        uint32_t w0 = (uint32_t)i | ((uint32_t)s.cur << 8) | ((uint32_t)std::max(1, s.have_refs) << 16);
        for (int r = 0; r < 3; r++) {
            // RefPicList0 entry r = the reference picture decoded ref_age[r] + 1 reference pictures ago (ring slot cur - 1 - age)
            w0 |= (uint32_t)dg_ref_slot(s, pic, r, ps->nbuf) << (10 + 2 * r);
        }
        w0 |= (pic.has_inter ? 1u << 24 : 0u) | (pic.has_intra ? 1u << 25 : 0u) | (filtered ? 1u << 26 : 0u) | (pic.deblock_idc == 0 ? 1u << 27 : 0u);
        T.w[0] = w0;
        T.w[1] = (uint32_t)(uint8_t)(int8_t)pic.cqo[0] | ((uint32_t)(uint8_t)(int8_t)pic.cqo[1] << 8) | ((uint32_t)(uint8_t)(int8_t)pic.filter_oa << 16) |
                 ((uint32_t)(uint8_t)(int8_t)pic.filter_ob << 24);
        // slices that are bands of whole rows run as independent wavefronts; any other shape: one wavefront over the picture.  The
        // filter sees one slice with idc 0 (edges between slices are filtered) and with slices that are no bands (k_dec_bs_pos has
        // zeroed the strengths between them where idc 2 says so)
        const int rows = pic.slice_rows > 0 ? pic.slice_rows : ps->mbh;
        const int frows = (pic.deblock_idc == 0 || pic.slice_rows < 0) ? ps->mbh : rows;
        T.w[2] = (uint32_t)rows; T.w[3] = recip32(rows);
        T.w[4] = (uint32_t)frows; T.w[5] = recip32(frows);
        T.w[6] = w6;
        any_join |= w6 != 0;   // (only now: a joining picture that was refused above makes no launch)
        s.recovery = pic.recovery;
        // the maps go on while they exist: a stream that concealed once and is strict again still refers to what it concealed
        if (s.loss || !s.taint.empty()) dg_damage(s, pic, ps->nbuf);
        else { s.tainted = s.concealed = s.gap = 0; s.joined = false; }
        any_inter |= pic.has_inter; any_intra |= pic.has_intra;
        if (filtered) { if (pic.has_intra) any_bs4 = true; else any_plain = true; }
        nbig += pic.big.size();
        if (outp) {
            if (npos == 0) for (int x = 0; x < S; x++) g->out.pics[oset][x] = out_no_pic(g->step_serial);
            int W, H;
            if (dg_out_size(s, W, H)) {   // (else: no picture of this stream in the output, and its report says why)
                const OutGeom geo = out_geom(g->out.layout, W, H, g->out.row_align);
                const size_t off = out_align(obytes, 256);
                dg_out_row(ocall, s, i, s.cur, W, H, geo, off, g->out.layout);
                g->out.pics[oset][i] = out_pic((int64_t)off, W, H, geo, 1, g->step_serial, dg_out_variant(s, g->out.layout));
                obytes = off + geo.bytes;
            }
        }
        pos_stream[npos++] = i;
    }
    if (npos == 0) return MI355X_H264_OK;
    // (armed: the output positions lie behind the DecPos rows and travel with them)
    uint8_t* const otab = outp ? g->out.h_tabx[k] + (size_t)S * sizeof(DecPos) : nullptr;
    const size_t otab_bytes = outp ? out_fill(ocall, otab) : 0;

    PicStore* const ps = &g->store;
    hipStream_t st = g->sync.st;
    const size_t nmb = (size_t)ps->nmb;
    int transfers = 0, launches = 0;
    // one transfer per array: the items from the lowest to the highest taking part
    end.queued_on = st;
    const int i0 = pos_stream[0], i1 = pos_stream[npos - 1];   // (positions are in stream order)
    for (int a = 0; a < DG_ARRAYS; a++) {
        if (a >= DG_MV4 && !any_inter) continue;
        const size_t off = (size_t)i0 * nmb * DG_BYTES[a], bytes = (size_t)(i1 - i0 + 1) * nmb * DG_BYTES[a];
        HIPCHK(g->err, hipMemcpyAsync(g->d_arr[a] + off, g->h_arr[k][a] + off, bytes, hipMemcpyHostToDevice, st));
        transfers++;
    }
    const DecPos* const d_tab = outp ? (const DecPos*)g->out.d_tabx : g->d_tab;
    const size_t tab_bytes = outp ? (size_t)S * sizeof(DecPos) + otab_bytes : (size_t)npos * sizeof(DecPos);
    HIPCHK(g->err, hipMemcpyAsync((void*)d_tab, tab, tab_bytes, hipMemcpyHostToDevice, st));
    transfers++;
    if (nbig) {   // the streams' large levels as one list, the indices counted from item 0
        static_assert(sizeof(h264dec::Picture::Big) == sizeof(DecBigLevel), "layout of the list of large levels");
        if (nbig > g->h_big_cap[k]) {   // (no upload out of this set is in flight: begin_step has waited)
            g->mem.drop(g->h_big[k]);
            g->h_big[k] = nullptr; g->h_big_cap[k] = 0;
            const size_t cap = nbig * 2 + 1024;
            HIPCHK(g->err, DM_PINNED(g->mem, g->h_big[k], cap * sizeof(DecBigLevel)));
            g->h_big_cap[k] = cap;
        }
        if (nbig > g->d_big_cap) {
            HIPCHK(g->err, hipStreamSynchronize(st));
            g->mem.drop(g->d_big);
            g->d_big = nullptr; g->d_big_cap = 0;
            const size_t cap = nbig * 2 + 1024;
            HIPCHK(g->err, DM_DEV(g->mem, g->d_big, cap * sizeof(DecBigLevel), false));
            g->d_big_cap = cap;
        }
        size_t at = 0;
        for (int p = 0; p < npos; p++) {
            const auto& big = g->st[pos_stream[p]].parser.picture().big;
            const uint32_t base = (uint32_t)((size_t)pos_stream[p] * nmb * LV_STRIDE);
            for (const auto& b : big) g->h_big[k][at++] = DecBigLevel{b.idx + base, b.val};
        }
        HIPCHK(g->err, hipMemcpyAsync(g->d_big, g->h_big[k], nbig * sizeof(DecBigLevel), hipMemcpyHostToDevice, st));
        transfers++;
    }
    HIPCHK(g->err, hipEventRecord(g->up_done[k], st));   // every copy out of the set has been queued
    end.launched = true;

    const dim3 wave(64);
    const unsigned NP = (unsigned)npos;
    if (any_join) {   // the grey reference pictures of the positions that join, ahead of everything that reads them
        DecRingFill F{};
        for (int p = 0; p < 3; p++) F.base[p] = ps->d_plane_base[p];
        F.st_y = ps->st_y; F.st_c = ps->st_c; F.st_ring_y = ps->st_ring_y; F.st_ring_c = ps->st_ring_c;
        F.vec_y = (unsigned)(nmb * 16); F.nbuf = ps->nbuf;
        hipLaunchKernelGGL(k_dec_ring_fill, dim3((F.vec_y + 255) / 256, 3, NP), dim3(256), 0, st, F, d_tab);
        launches++;
    }
    {
        const int words = (int)(nmb * (LV_STRIDE / 4));
        hipLaunchKernelGGL(k_dec_widen_pos, dim3((words + 255) / 256, NP), dim3(256), 0, st, (const uint32_t*)g->d_arr[DG_LV8], (const MbInfo*)ps->d_mb, ps->d_levels, (int)nmb,
                           d_tab);
        launches++;
        if (nbig) { hipLaunchKernelGGL(k_dec_patch, dim3(((int)nbig + 255) / 256), dim3(256), 0, st, (const DecBigLevel*)g->d_big, (int)nbig, ps->d_levels); launches++; }
    }
    FrameParams P = store_frame_params(ps);
    P.w = ps->cw; P.h = ps->ch;
    P.nref = 1;
    for (int p = 0; p < 3; p++) P.rec[p] = ps->d_plane_base[p];   // (the positions' planes and references: from the table)
    P.st_ring_y = ps->st_ring_y; P.st_ring_c = ps->st_ring_c; P.nbuf = ps->nbuf;
    P.sl.rows = ps->mbh; P.sl.inv = recip32(ps->mbh);
    P.band.row0 = 0; P.band.rows = ps->mbh;
    P.mbqp = g->d_arr[DG_QP]; P.mv4 = (const int16_t*)g->d_arr[DG_MV4]; P.refq = g->d_arr[DG_REFQ]; P.mbavail = g->d_arr[DG_AVAIL];
    P.dectab = d_tab;
    unsigned* const h_err = g->sync.h_err;
    if (any_inter) {
        hipLaunchKernelGGL(k_dec_inter_pos, dim3(ps->nmb, NP), wave, 0, st, P);
        hipLaunchKernelGGL(k_dec_resid, dim3((ps->nmb + 3) / 4, NP), wave, 0, st, P);
        launches += 2;
    }
    if (any_intra) {
        const IntraRowParams R = intra_row_params(ps, P, h_err, npos);
        hipLaunchKernelGGL((k_pintra_rows<true, true>), dim3(ps->mbh, std::min(NP, (unsigned)g->intra_slots)), wave, 0, st, R);
        launches++;
    }
    if (any_plain || any_bs4) {
        const unsigned db_serial = next_nonzero(ps->serial);
        DecBsParams B{};
        B.mb = ps->d_mb; B.mv4 = (const int16_t*)g->d_arr[DG_MV4]; B.refq = g->d_arr[DG_REFQ]; B.bs = (uint8_t*)ps->d_bs; B.mbw = ps->mbw; B.nmb = ps->nmb; B.mbdiv = P.mbdiv;
        B.mbavail = g->d_arr[DG_AVAIL];
        hipLaunchKernelGGL(k_dec_bs_pos, dim3((ps->nmb + 1) / 2, NP), wave, 0, st, B, ps->d_anybs, db_serial, d_tab);
        launches++;
        // always the per-edge thresholds; the form with the bS 4 filter for the positions with intra macroblocks, the one without
        // for the others (the pair of launches of the encoder's P steps, chosen by the table's flags)
        DbParams D = db_params(ps, ps->d_plane_base, P.sl, 26);
        D.mbqp = g->d_arr[DG_QP];
        DbRowParams R = db_row_params(ps, D, h_err, db_serial, P.pic_serial, 0, npos);
        R.st_ring_y = ps->st_ring_y; R.st_ring_c = ps->st_ring_c; R.dectab = d_tab;
        const dim3 grid(ps->mbh, std::min(NP, (unsigned)g->filter_slots));
        if (any_plain) { R.need_intra = -1; hipLaunchKernelGGL((k_deblock_rows<false, true, true>), grid, wave, 0, st, R); launches++; }
        if (any_bs4) { R.need_intra = 1; hipLaunchKernelGGL((k_deblock_rows<true, true, true>), grid, wave, 0, st, R); launches++; }
    }
    HIPCHK(g->err, hipGetLastError());
    if (outp) {
        // behind the loop filter, and ahead of the next step on this stream, which may write the very ring slot (a non-reference
        // picture leaves `cur` where it was): the step's pictures into the staging buffer, and that into the pinned set
        // (a step none of whose pictures can be delivered at the size asked for makes neither: its set says "no picture" for all)
        if (ocall.n) {
            HIPCHK(g->err, out_launch(ps, g->out.layout, ocall, otab, g->out.d_tabx + (size_t)S * sizeof(DecPos), g->out.rd.d_stage, st));
            HIPCHK(g->err, hipMemcpyAsync(g->out.h_set[oset], g->out.rd.d_stage, obytes, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(g->err, hipEventRecord(g->out.done[oset], st));
        g->out.cur = oset; g->out.count = std::min(2, g->out.count + 1);
        g->last[7] = g->last[8] = ocall.n ? 1 : 0;
    }
    g->busy = true;
    g->nflight = npos;
    for (int p = 0; p < npos; p++) g->flight[p] = pos_stream[p];
    for (int p = 0; p < npos; p++) {   // parser and ring take the picture in together
        const int i = pos_stream[p];
        DecGroupStream& s = g->st[i];
        const bool is_ref = s.parser.picture().is_ref;
        s.last = s.cur;
        s.last_serial = g->step_serial;
        s.parser.commit();
        if (is_ref && !s.virt) {   // sliding window (8.2.5.3)
            s.cur = (s.cur + 1) % ps->nbuf;
            s.have_refs = std::min(s.have_refs + 1, std::min(s.max_refs, ps->nbuf - 1));
        } else if (is_ref) {       // the same window over the list of slots: the next picture goes to a slot no held picture lies in
            s.refs.push(s.cur, false);
            s.have_refs = std::min(s.have_refs + 1, std::min(s.max_refs, ps->nbuf - 1));
            s.cur = s.refs.next_free(s.cur, s.have_refs, ps->nbuf);
        }
        s.since++;
        s.pictures++;
        got[i] = 1;
    }
    g->last[1] = npos; g->last[2] = launches; g->last[3] = transfers;
    static const bool no_lookahead = getenv("MI355X_H264_DEC_SYNC") != nullptr;   // (measurements: wait for every step before returning)
    int wrc = MI355X_H264_OK;
    if (no_lookahead) wrc = dg_wait(g);
    g->last_ms[1] = now_ms() - t1;
    g->last[6] = (int64_t)(g->last_ms[1] * 1e3);
    if (wrc) for (int p = 0; p < npos; p++) { got[pos_stream[p]] = 0; rc[pos_stream[p]] = wrc; }
    return wrc;
}

int64_t dg_read(mi355x_h264_dec_group* g, int stream, void* dst, size_t cap, bool to_device)
{
    if (!g || !dst || stream < 0 || stream >= g->nstreams || g->st[stream].last < 0) return MI355X_H264_E_ARG;
    const DecGroupStream& s = g->st[stream];
    const size_t w = (size_t)s.width, h = (size_t)s.height, need = w * h * 3 / 2;
    if (cap < need) return MI355X_H264_E_ARG;
    if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
    if (const int wrc = dg_wait(g)) return wrc;   // the picture asked for may still be in flight
    const PicStore* const ps = &g->store;
    uint8_t* o = (uint8_t*)dst;
    const hipMemcpyKind kind = to_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int p = 0; p < 3; p++) {
        const size_t pw = p ? w / 2 : w, ph = p ? h / 2 : h, pitch = p ? (size_t)ps->cw / 2 : (size_t)ps->cw;
        const uint8_t* plane = ps->d_plane_base[p] + (size_t)stream * (p ? ps->st_c : ps->st_y) + (size_t)s.last * (p ? ps->st_ring_c : ps->st_ring_y);
        const uint8_t* src = plane + (size_t)(p ? s.crop_y / 2 : s.crop_y) * pitch + (size_t)(p ? s.crop_x / 2 : s.crop_x);
        if (hipMemcpy2D(o, pw, src, pitch, pw, ph, kind) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipMemcpy2D");
        o += pw * ph;
    }
    return (int64_t)need;
}

// every stream's last picture in one launch (and, to the host, one transfer)
int64_t dg_read_all(mi355x_h264_dec_group* g, int layout, int row_align, void* dst, size_t cap, bool to_device, mi355x_h264_dec_out_pic* pics)
{
    if (!g || !pics || !out_args_ok(layout, row_align)) return MI355X_H264_E_ARG;
    OutCall call;
    mi355x_h264_dec_out_pic desc[DEC_GROUP_MAX_STREAMS];
    size_t total = 0;
    for (int i = 0; i < g->nstreams; i++) {
        DecGroupStream& s = g->st[i];
        desc[i] = out_no_pic(g->step_serial);
        if (s.last < 0) continue;
        int W, H;
        if (!dg_out_size(s, W, H)) continue;   // (its report says why; the others are delivered)
        const OutGeom geo = out_geom(layout, W, H, row_align);
        const size_t off = out_align(total, 256);
        dg_out_row(call, s, i, s.last, W, H, geo, off, layout);
        desc[i] = out_pic((int64_t)off, W, H, geo, s.last_serial == g->step_serial, g->step_serial, dg_out_variant(s, layout));
        total = off + geo.bytes;
    }
    const int n = call.n;
    if (n == 0) return MI355X_H264_E_ARG;
    if (dst && (cap < total || (to_device && ((uintptr_t)dst & 15)))) return MI355X_H264_E_ARG;
    memcpy(pics, desc, (size_t)g->nstreams * sizeof(desc[0]));
    if (!dst) return (int64_t)total;
    if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
    if (const int wrc = dg_wait(g)) return wrc;   // the pictures asked for may still be in flight
    const PicStore* const ps = &g->store;
    hipStream_t st = g->sync.st;
    HIPCHK(g->err, hipStreamSynchronize(st));   // (an armed step's copy out of the staging buffer; nothing else is queued)
    DecOutBuf& b = g->out.rd;
    if (out_reserve(g->mem, b, to_device ? 0 : total, to_device ? 0 : total) != hipSuccess)
        return set_err(g->err, MI355X_H264_E_NOMEM, "memory for the output staging (%s)", t_failed_call);
    out_fill(call, b.h_tab);
    g->last[9] = g->last[10] = 0;
    HIPCHK(g->err, out_launch(ps, layout, call, b.h_tab, b.d_tab, to_device ? (uint8_t*)dst : b.d_stage, st));
    g->last[9] = 1;
    if (!to_device) { HIPCHK(g->err, hipMemcpyAsync(b.h_stage, b.d_stage, total, hipMemcpyDeviceToHost, st)); g->last[10] = 1; }
    HIPCHK(g->err, hipStreamSynchronize(st));
    if (!to_device) memcpy(dst, b.h_stage, total);
    return (int64_t)total;
}

int dg_set_output(mi355x_h264_dec_group* g, int layout, int row_align)
{
    if (!g) return MI355X_H264_E_ARG;
    if (layout == -1) { g->out.armed = false; g->out.count = 0; g->last[7] = g->last[8] = 0; return MI355X_H264_OK; }
    if (!out_args_ok(layout, row_align)) return MI355X_H264_E_ARG;
    if (g->store.made()) {   // the sets may be made anew for this layout by the next step: nothing may be on its way into them
        if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
        if (const int wrc = dg_wait(g)) return wrc;
        HIPCHK(g->err, hipStreamSynchronize(g->sync.st));
    }
    g->out.armed = true; g->out.ready = false; g->out.layout = layout; g->out.row_align = row_align; g->out.count = 0;
    return MI355X_H264_OK;
}

int dg_output(mi355x_h264_dec_group* g, int back, const uint8_t** data, mi355x_h264_dec_out_pic* pics)
{
    if (!g || !data || !pics || back < 0 || back > 1 || !g->out.armed || g->out.count <= back) return MI355X_H264_E_ARG;
    const int o = back ? g->out.cur ^ 1 : g->out.cur;
    if (back == 0) {   // (the step before it was waited for when the last one was launched)
        if (hipSetDevice(g->device) != hipSuccess) return set_err(g->err, MI355X_H264_E_HIP, "hipSetDevice");
        HIPCHK(g->err, hipEventSynchronize(g->out.done[o]));
        if (const int wrc = dg_wait(g)) return wrc;
    }
    *data = g->out.h_set[o];
    memcpy(pics, g->out.pics[o], (size_t)g->nstreams * sizeof(pics[0]));
    return MI355X_H264_OK;
}

}  // namespace
