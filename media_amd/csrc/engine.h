// media_amd/csrc/engine.h -- the encoder engine behind include/mi355x_h264.h: device memory, streams, access-unit
// slots, one lockstep step of launches (submit_step), the wait for it and the host's finish of every access unit.  An engine is
// a picture store (pic_store.h: ring, per-macroblock arrays, hand-off granules, flags, serials) plus what coding a stream takes.
// The stream hub (hub.h) drives one engine; the decoder groups (dec_group.h) own a store and no engine.  Part of the one
// translation unit mi355x_h264.hip, which includes the kernels before this file.
#pragma once

namespace {

constexpr int NSLOT = 3;          // access-unit slots in flight

// where the access units of a step lie in a slot's h_au: offset of the first byte and of the slice payload; their type; and the
// step's quality report.  What is the picture's own (layer, QP, refresh band) is in its ItemPic
struct AuLayout { size_t au_start = 0, payload_off = 0; bool idr = false;
                  int quality = 0;      // quality report of the step's pictures: 0 off, 1 compared (k_sse ran), 2 on but nothing to compare
                  int ssim = 0; };      // the SSIM record accompanies it (compared: k_ssim ran behind k_sse)

struct Slot {
    uint32_t* d_bitbuf = nullptr;   // device slice payload (zeroed before use)
    SliceInfo* d_info = nullptr;
    SliceInfo* h_info = nullptr;    // pinned
    uint8_t* h_au = nullptr;        // pinned access unit buffer
    AuLayout lay;                   // of the picture in flight
    ItemPic pics[MAX_BATCH];        // and its records, one per batch item (direct steps; the stream hub's are the gathered step's)
    unsigned long long* h_qpart = nullptr;   // quality report (pinned, with the first enable): [G][mbh][SSE_SEGS][3] plane sums per wave of k_sse
    uint32_t* h_qmap = nullptr;              //   and [G][nmb] sums per macroblock, stored by k_sse; rows outside the band stay 0
    long long* h_spart = nullptr;            // SSIM (pinned, with the first enable that asks for it): [G][mbh][SSIM_SEGS][3] plane sums per wave of k_ssim
    int32_t* h_smap = nullptr;               //   and [G][nmb] luma sums per macroblock, stored by k_ssim; rows outside the band stay 0
    bool busy = false;
    StepSync sync;                  // on the engine's stream pair
    // stats events of this frame: pairs (start, stop, kernel id, launches, mbs)
    struct Ev { hipEvent_t a, b; int k; uint32_t launches, mbs; };
    std::vector<Ev> evs;
};

}  // namespace

struct mi355x_h264_encoder : PicStore {      // (G: the lockstep batch, closed GOPs / streams encoded together; nbuf = nrefs + 1)
    mi355x_h264_config cfg{};
    int level_idc = 0;
    int nsl = 1;                             // slices per picture: bands of sl.rows macroblock rows
    SliceRows sl{};
    size_t slice_cap = 0;                    // bytes of payload buffer per slice (multiple of 16)
    // slice bands over several GPUs: this instance codes slices b_sl0 .. b_sl0 + b_nsl - 1 = rows b_row0 .. b_row0 + b_rows - 1
    int b_sl0 = 0, b_nsl = 1, b_row0 = 0, b_rows = 0, b_nmb = 0;
    size_t st_bitbuf_bytes = 0, st_au = 0;   // per-item strides
    hipStream_t stream = nullptr;
    hipStream_t stream_ec = nullptr;         // entropy coding runs here, beside the deblocking wavefront (= stream when the process holds many engines)
    std::atomic<int>* counted_live = nullptr;
    enum { MAX_REFS = MAX_BUF - 1 };
    int nrefs = 1;                           // reference frames searched (config.refs); in the ring `cur` is written, cur - 1 - r (mod nbuf) is ref_idx_l0 r
    QpEntry* d_qtab = nullptr;               // [52] quantiser constants by QP (indirect launches)
    int nslots = NSLOT;                      // access-unit slots allocated (the hub's engine needs one)
    uint8_t* d_pre[3] = {nullptr};           // copy of the reconstruction before the loop filter (debug)
    PicSeq seq;                              // seq.cur: index written by the picture being encoded
    bool pair_filter = true;                 // two macroblock rows per wave in the loop filter for lockstep batches of pair_min_batch pictures or more
    int pair_min_batch = 8;                  // (MI355X_H264_PAIR_FILTER=N sets it, 0 turns the pair form off)
    int16_t* d_mvd = nullptr;
    uint32_t* d_me_total = nullptr;          // [G][nmb] best motion cost so far over the reference pictures (k_me, one launch each)
    int* d_pmv = nullptr;                    // [G][nmb] the previous picture's vectors, parked for the later launches - and, temporal layers, by a layer-1 picture for the layer-0 picture behind it
    int last_layer = 0;                      // temporal layer of the last finished picture (mi355x_h264_last_temporal_id)
    std::vector<int> last_rband;             // per batch item: all-intra band of its last finished picture, -1 none (mi355x_h264_last_refresh_band)
    uint16_t* d_slotbits = nullptr;
    unsigned long long* d_slotcode = nullptr;
    uint32_t* d_mbbits = nullptr;
    int32_t* d_prevcoded = nullptr;          // [G][nmb + 1] skip-run helper (k_skip_scan)
    uint16_t* d_me_cost = nullptr;           // [G][nmb] per-macroblock motion cost (scene-change statistic)
    std::vector<uint32_t> last_me_cost;      // of the last finished picture, per batch item
    bool diag_mode = false;                  // debug: one launch per wavefront step instead
    uint8_t* d_stage = nullptr;              // device copy of a host-supplied picture
    uint8_t* h_stage = nullptr;              // pinned staging for strided host input
    const uint8_t* last_src = nullptr;       // where the kernels read the last picture (MI355X_H264_DBG_SRC serves it when that is d_stage)
    uint8_t* d_rgba = nullptr, *h_rgba = nullptr;   // RGBA pictures on their way to the conversion kernel (allocated with the first)
    uint8_t* d_inject_src = nullptr;         // mi355x_h264_debug_code_syntax: the batch items' source pictures (allocated with the first call)
    size_t frame_bytes = 0, bitbuf_cap = 0, au_cap = 0;
    Slot slots[NSLOT];
    int next_slot = 0;
    StreamShape shape{};                     // what the parameter sets and slice headers are written from
    ColourDesc colour;                       // the description the engine was created with (mi355x_h264_create_colour, the hub's); none: BT.601 limited, no VUI
    std::vector<uint8_t> sps_pps;            // Annex-B SPS + PPS NALs
    std::vector<std::vector<uint8_t>> esc_buf;  // slow path: escaped access unit, per batch item
    int idr_step = 1;                        // idr_pic_id stride between the batch items
    bool after_injected = false;             // the last picture came through mi355x_h264_debug_code_syntax
    int qp = 26;
    bool keep_pre = false, stats_on = false;
    std::vector<hipEvent_t> ev_pool;
    int me_turn = 0;                         // this engine's id at the GPU's motion-search lock (0: takes no part)
    uint32_t p_intra_x16 = 0;                // intra macroblocks per P picture, recent pictures (x 16, a running mean): sizes k_pintra_rows' grid
    mi355x_h264_stats stats{};
    // quality report (mi355x_h264_quality_enable; everything below comes with the first enable)
    bool quality_on = false;
    hipEvent_t q_ready = nullptr;            // the reconstruction of the step being launched is final: k_sse may start on the second stream
    hipEvent_t q_done[MAX_BUF] = {nullptr};  // direct steps: behind the k_sse that compared ring slot b
    bool q_done_set[MAX_BUF] = {false};
    std::vector<mi355x_h264_quality> q_item; // [G] record of the item's last finished picture
    std::vector<const uint32_t*> q_map;      // [G] its map, in the pinned memory of the slot that carried it (null: nothing compared)
    std::vector<uint8_t> q_have;             // [G] the item has a record
    std::vector<mi355x_h264_quality> q_recs; // the records of the last call, in the order of sizes[]: item g's goes to g * q_mul + q_add
    size_t q_mul = 1, q_add = 0;
    // SSIM beside the SSE (mi355x_h264_quality_enable_ex with MI355X_H264_QUALITY_SSIM; allocated with the first enable that asks for it)
    bool ssim_on = false, ssim_ready = false;
    std::vector<mi355x_h264_ssim> s_item;    // [G] as q_item
    std::vector<const int32_t*> s_map;       // [G] as q_map
    std::vector<uint8_t> s_have;             // [G] the item has an SSIM record
    std::vector<mi355x_h264_ssim> s_recs;    // as q_recs, same order
    char err[256] = {0};
};

// ---------------------------------------------------------------------------------------------------------------
// One motion search of a lockstep batch at a time per GPU.
// Two instances beside each other are worth more than one because the dependency-bound kernels of one (loop filter, entropy
// coding, row wavefronts) run in the issue slots the other's motion search leaves.  Left to themselves the instances settle in
// whatever phase their first steps put them - search beside filter (good), or search beside search and filter beside filter (2 - 5 %
// less, run by run: section 7 of DESIGN.md).  A lock word in device memory per GPU keeps the searches apart: a one-wave kernel in
// front of a search takes it (compare-and-swap, sleeping between tries), and behind the search it is given back: by the first wave
// of k_tq, the kernel that follows the search on the same stream (k_tq.h tq_turn_release: the lock and the id travel in its
// FrameParams; a launch of its own for that one compare-and-swap cost a kernel boundary on every P step's chain), or - High profile,
// where k_tq8 follows - by the one-thread kernel k_turn_release in front of k_tq8 (the release from inside k_tq8 measured SLOWER
// than the launch, in every run: DESIGN.md section 11).
// Whoever comes first goes first - no order is imposed, so an engine in its IDR step, or gone, holds nobody up (an ORDER between the
// engines' searches, by events or by counters, follows the order in which the host threads happened to queue them and left one
// instance idle for 1.4 ms of every step) - and the holder's search and the release behind it (k_turn_release, or the k_tq that
// carries the lock) are queued right behind its acquire, in the same submit_step and with no early return between them, so the
// lock is always given back; the wait gives up after TURN_TIMEOUT_US all the same.
// ---------------------------------------------------------------------------------------------------------------
// -DTURN_AB_COUNT (measurement build, make ab): acquires that ended by the time-out instead of by getting the lock - a release that
// went missing would show here; the host reads and clears the word with mi355x_h264_turn_timeouts().
#ifdef TURN_AB_COUNT
__device__ unsigned g_turn_timeouts;
extern "C" __attribute__((visibility("default"))) int mi355x_h264_turn_timeouts(unsigned* out, int clear)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_turn_timeouts), sizeof(unsigned)) != hipSuccess) return -1;
    const unsigned zero = 0;
    if (clear && hipMemcpyToSymbol(HIP_SYMBOL(g_turn_timeouts), &zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#define TURN_COUNT_TIMEOUT() atomicAdd(&g_turn_timeouts, 1u)
#else
#define TURN_COUNT_TIMEOUT() ((void)0)
#endif
__global__ void k_turn_acquire(unsigned* lock, unsigned id, int timeout_us)
{
    if (threadIdx.x) return;
    const long long t0 = wall_clock64();   // 100 MHz
    for (;;) {
        unsigned expect = 0u;
        if (__hip_atomic_compare_exchange_strong(lock, &expect, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if (wall_clock64() - t0 > (long long)timeout_us * 100) { TURN_COUNT_TIMEOUT(); __hip_atomic_store(lock, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
        __builtin_amdgcn_s_sleep(16);
    }
}
__global__ void k_turn_release(unsigned* lock, unsigned id)
{
    unsigned expect = id;
    (void)__hip_atomic_compare_exchange_strong(lock, &expect, 0u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

namespace {
enum { TURN_MIN_BATCH = 16, TURN_DEVICES = 16, TURN_TIMEOUT_US = 3000 };
struct MeTurns {
    std::mutex mu;
    unsigned* d_lock[TURN_DEVICES] = {};   // allocated with the first engine of the device, kept for the life of the process
    unsigned next_id = 1;
};
MeTurns g_turns;
const bool g_turns_on = !(getenv("MI355X_H264_ME_TURNS") && atoi(getenv("MI355X_H264_ME_TURNS")) == 0);

enum { PINTRA_SPARSE_MBS = 8 };   // intra macroblocks per P picture up to which k_pintra_rows takes the step's pictures one after the other
}  // namespace

namespace {

int avail_refs(const mi355x_h264_encoder* e, bool idr) { return e->seq.avail_refs(idr, e->nrefs); }
inline bool mb_is_intra_host(int type) { return type == MB_I16 || type == MB_IPCM || type == MB_I4; }

hipEvent_t get_event(mi355x_h264_encoder* e)
{
    if (!e->ev_pool.empty()) { hipEvent_t ev = e->ev_pool.back(); e->ev_pool.pop_back(); return ev; }
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

struct StatScope {
    mi355x_h264_encoder* e; Slot* s; int k; uint32_t launches, mbs; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    StatScope(mi355x_h264_encoder* e_, Slot* s_, int k_, uint32_t l, uint32_t m, hipStream_t st_ = nullptr)
        : e(e_), s(s_), k(k_), launches(l), mbs(m), st(st_ ? st_ : e_->stream)
    {
        if (e->stats_on) { a = get_event(e); b = get_event(e); if (a) (void)hipEventRecord(a, st); }
    }
    ~StatScope()
    {
        if (e->stats_on && a && b) { (void)hipEventRecord(b, st); s->evs.push_back({a, b, k, launches, mbs}); }
    }
};

// ---- one lockstep step: which pictures, where from, on which streams ----
// Position k of the grid is picture items[k]: its batch item, ring slot, QP, frame_num, idr_pic_id, reference count, layer and
// refresh band (ItemPic, made by PicSeq::pic), whoever brings the step.  Direct (d_itemtab == nullptr): the n = e->G batch items of the
// encoder in their order, one stream state, consecutive idr_pic_ids - the closed-GOP batch of mi355x_h264_encode_gops_device and the
// single-picture calls; the kernels find item g at g strides.  Indirect (the stream hub below): the kernels are the IND = true
// instantiations and read each position's facts from d_itemtab (item_word.h), and the source picture of position k lies at
// d_srctab[k] (d_src is not used) - wherever that is: a slot of the hub's staging array or the caller's own device memory.  A step
// holds pictures of ONE type (IDR or P): the two run different kernels.  A P step's positions are ordered by their pictures' number
// of reference pictures (ItemPic.nref, most first): k_me's launch for reference picture r covers the positions that have it, the first ones.
// mi355x_h264_debug_code_syntax: the decisions of the step's pictures come from the host (arrays of n items) instead of the
// decision and reconstruction kernels
struct Injected { const void* mbinfo; const void* levels; const void* mvq; const void* mbaux; };
struct Step {
    const uint8_t* d_src = nullptr; size_t src_item_stride = 0; bool nv12 = false; bool idr = false;
    int n = 1;
    const ItemPic* items = nullptr;   // [n]
    const uint32_t* d_itemtab = nullptr;
    const unsigned long long* d_srctab = nullptr;
    const StepSync* sync = nullptr;   // streams, events and the time-out flag of the step
    bool one_stream = false;          // entropy coding stays on sync->st
    Slot* slot = nullptr;   // payload / access-unit buffers (laid out by batch item) and, with stats on, the event list
    const Injected* inj = nullptr;   // test hook (direct steps only): upload these instead of deciding and reconstructing; no loop filter
    AuLayout lay;   // out: where the access units lie in slot->h_au
};

#define LAUNCH2(ind, KT, KF, grid, block, stream, ...)                                   \
    do {                                                                                 \
        if (ind) hipLaunchKernelGGL(KT, grid, block, 0, stream, __VA_ARGS__);            \
        else hipLaunchKernelGGL(KF, grid, block, 0, stream, __VA_ARGS__);                \
    } while (0)

// the store's part of the frame parameters and what the encoder's kernels (motion search, entropy coding) take besides
FrameParams frame_params(mi355x_h264_encoder* e)   // takes the next picture serial
{
    FrameParams P = store_frame_params(e);
    P.mvd = e->d_mvd; P.me_cost = e->d_me_cost; P.me_total = e->d_me_total; P.pmv = e->d_pmv;
    return P;
}

// ---- the stages of a step, in the order submit_step calls them.  A stage queues its launches on the stream it names; the events
// between the two streams are submit_step's alone.  ind: the IND = true kernels run (device tables exist) ----

// The step's FrameParams (takes the next picture serial) and me_pos[r] = the positions that have reference picture r, k_me's grid
// for it (the kernels take each position's own count from its itemtab word).  Refuses positions out of the order of their counts
int step_frame_params(mi355x_h264_encoder* e, const Step& T, FrameParams& P, int* me_pos)
{
    const bool idr = T.idr, ind = T.d_itemtab != nullptr;
    P = frame_params(e);
    P.src = T.d_src; P.src_nv12 = T.nv12 ? 1 : 0; P.w = e->cfg.width; P.h = e->cfg.height;
    for (int k = 0; k < T.n; k++) {
        const int nr = T.items[k].nref;
        if (nr < (idr ? 0 : 1) || nr > (idr ? 0 : e->nrefs) || (k > 0 && nr > T.items[k - 1].nref))
            return set_err(e->err, MI355X_H264_E_INTERNAL, "step position %d: %d reference pictures (after %d)", k, nr, k ? T.items[k - 1].nref : 0);
        for (int r = 0; r < nr; r++) me_pos[r]++;
    }
    P.nref = std::max(1, T.items[0].nref);   // the most any position has
    const int cur = ind ? 0 : T.items[0].cur;   // direct: the ring slot every item writes (indirect: plane bases; the position's slot is in its word)
    for (int p = 0; p < 3; p++) {
        P.rec[p] = ind ? e->d_plane_base[p] : e->d_planes[cur][p];
        for (int r = 0; r < mi355x_h264_encoder::MAX_REFS; r++) P.refs[r][p] = e->d_planes[(cur + e->nbuf - 1 - std::min(r, e->nrefs - 1)) % e->nbuf][p];
        P.ref[p] = P.refs[0][p];
    }
    // (temporal layers, and intra refresh: the other form of k_me and the picture's band; indirect launches: the position's own word)
    P.me = ind ? 0 : me_word(T.items[0], e->shape.refresh != 0);
    P.itemtab = T.d_itemtab; P.srctab = T.d_srctab; P.qtab = e->d_qtab; P.st_ring_y = e->st_ring_y; P.st_ring_c = e->st_ring_c; P.nbuf = e->nbuf;
    P.st_src = T.src_item_stride; P.sl = e->sl;
    P.band.row0 = e->b_row0; P.band.rows = e->b_rows;
    fill_qp(P.qy, P.qc, P.lambda, P.sad_nz, e->qp);   // (indirect launches take these from qtab by the item's own QP)
    P.search = e->cfg.search;
    return MI355X_H264_OK;
}

// mi355x_h264_debug_code_syntax: the arrays k_i4_decide / k_intra_rows / k_me / k_tq / k_pintra_rows would have left, and the flags
// they would have raised
int step_inject(mi355x_h264_encoder* e, const Step& T, const FrameParams& P)
{
    hipStream_t st = T.sync->st;
    const size_t n = (size_t)T.n * e->nmb;
    HIPCHK(e->err, hipMemcpyAsync(e->d_mb, T.inj->mbinfo, n * sizeof(MbInfo), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemcpyAsync(e->d_levels, T.inj->levels, n * LV_STRIDE * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemcpyAsync(e->d_mvq, T.inj->mvq, n * 8 * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemcpyAsync(e->d_aux, T.inj->mbaux, n * 16, hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemsetAsync(e->d_me_cost, 0, n * sizeof(uint16_t), st));
    unsigned anypcm[MAX_BATCH] = {}, anyintra[MAX_BATCH] = {}, stepintra = 0;
    const MbInfo* m = (const MbInfo*)T.inj->mbinfo;
    for (int g = 0; g < T.n; g++)
        for (int i = 0; i < e->nmb; i++) {
            const int type = m[(size_t)g * e->nmb + i].type;
            if (type == MB_IPCM) anypcm[g] = P.pic_serial;
            if (!T.idr && mb_is_intra_host(type)) anyintra[g] = stepintra = P.pic_serial;
        }
    HIPCHK(e->err, hipMemcpyAsync(e->d_anypcm, anypcm, (size_t)T.n * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemcpyAsync(e->d_anyintra, anyintra, (size_t)T.n * sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipMemcpyAsync(e->d_stepintra, &stepintra, sizeof(unsigned), hipMemcpyHostToDevice, st));
    HIPCHK(e->err, hipStreamSynchronize(st));   // (the flag arrays live on this stack)
    return MI355X_H264_OK;
}

// IDR pictures: decide, then the row wavefront
void step_recon_idr(mi355x_h264_encoder* e, const Step& T, const FrameParams& P)
{
    const bool ind = T.d_itemtab != nullptr;
    const unsigned G = (unsigned)T.n;
    hipStream_t st = T.sync->st;
    StatScope sc(e, T.slot, MI355X_H264_K_INTRA, (uint32_t)(e->diag_mode ? e->mbw + e->mbh - 1 : 1), (uint32_t)(e->b_nmb * T.n), st);
    LAUNCH2(ind, k_i4_decide<true>, k_i4_decide<false>, dim3((e->b_nmb + 3) / 4, G), dim3(64), st, P, 0);   // Intra4x4 or Intra16x16, and the block modes: from the source alone
    if (e->diag_mode && !ind) {
        for (int s = 0; s < e->mbw + e->mbh - 1; s++) {
            const int ymin = std::max(0, s - e->mbw + 1), ymax = std::min(e->mbh - 1, s);
            hipLaunchKernelGGL(k_intra_diag, dim3(ymax - ymin + 1, G), dim3(64), 0, st, P, s);
        }
        return;
    }
    const IntraRowParams R = intra_row_params(e, P, T.sync->h_err, (int)G);
    // MI355X_H264_INTRA_SLOTS: pictures the row wavefront holds at a time (k_intra_rows)
    static const int slots = getenv("MI355X_H264_INTRA_SLOTS") ? std::max(1, atoi(getenv("MI355X_H264_INTRA_SLOTS"))) : 24;
    LAUNCH2(ind, k_intra_rows<true>, k_intra_rows<false>, dim3(e->b_rows, std::min(G, (unsigned)slots)), dim3(128), st, R);
}

// P pictures: the motion search behind the GPU's lock (one launch per reference picture), transform and quantisation, the intra pass.
// (P: the lock travels in it for the launch of k_tq alone)
void step_recon_p(mi355x_h264_encoder* e, const Step& T, FrameParams& P, const int* me_pos)
{
    const bool ind = T.d_itemtab != nullptr, rfr = e->shape.refresh != 0;
    const unsigned G = (unsigned)T.n;
    hipStream_t st = T.sync->st;
    const bool turns = g_turns_on && !ind && e->me_turn > 0 && T.n >= TURN_MIN_BATCH;
    if (turns) hipLaunchKernelGGL(k_turn_acquire, dim3(1), dim3(64), 0, st, g_turns.d_lock[e->device], (unsigned)e->me_turn, (int)TURN_TIMEOUT_US);
    { StatScope sc(e, T.slot, MI355X_H264_K_ME, (uint32_t)P.nref, (uint32_t)(e->b_nmb * T.n), st);
      FrameParams Q = P;   // one launch per reference picture (config.refs): Q.ref = the planes of ref_idx_l0 = Q.rf
      Q.rf_last = P.nref - 1;
      for (int r = 0; r < P.nref; r++) {   // (over the positions that have the picture: no launch places a wave that has nothing to do)
          Q.rf = r;
          for (int p = 0; p < 3; p++) Q.ref[p] = P.refs[r][p];
          if (rfr) LAUNCH2(ind, (k_me<true, true>), (k_me<false, true>), dim3(e->b_nmb, (unsigned)me_pos[r]), dim3(64), st, Q);
          else LAUNCH2(ind, k_me<true>, k_me<false>, dim3(e->b_nmb, (unsigned)me_pos[r]), dim3(64), st, Q);
      } }
    // the lock goes back with the first wave of the k_tq that follows on this stream (k_tq.h tq_turn_release); in front of k_tq8
    // by a launch of its own
    if (turns && e->cfg.profile_idc == 100) hipLaunchKernelGGL(k_turn_release, dim3(1), dim3(1), 0, st, g_turns.d_lock[e->device], (unsigned)e->me_turn);
    else if (turns) { P.turn_lock = g_turns.d_lock[e->device]; P.turn_id = (unsigned)e->me_turn; }
    { StatScope sc(e, T.slot, MI355X_H264_K_PMB, 1, (uint32_t)(e->b_nmb * T.n), st);
      if (e->cfg.profile_idc == 100) LAUNCH2(ind, k_tq8<true>, k_tq8<false>, dim3((e->b_nmb + 15) / 16, G), dim3(64), st, P);   // High: 8x8 transform, sixteen macroblocks per wave
      else LAUNCH2(ind, k_tq<true>, k_tq<false>, dim3((e->b_nmb + 7) / 8, G), dim3(64), st, P);   // one wave per eight macroblocks
      P.turn_lock = nullptr; }   // (given back: no later launch of the step carries it)
    // macroblocks the motion search handed to the intra pass (returns at once when there are none)
    const IntraRowParams R = intra_row_params(e, P, T.sync->h_err, (int)G);
    // The grid holds ONE picture at a time (the workgroups walk the step's pictures) while the recent P pictures had next to
    // no intra macroblocks, all of them once they have: see k_pintra_rows.  MI355X_H264_PINTRA_SLOTS fixes the number.
    static const int pslots_env = getenv("MI355X_H264_PINTRA_SLOTS") ? std::max(1, atoi(getenv("MI355X_H264_PINTRA_SLOTS"))) : 0;
    const unsigned pslots = std::min(G, pslots_env ? (unsigned)pslots_env : (e->p_intra_x16 > 16u * PINTRA_SPARSE_MBS ? G : 1u));
    if (ind) {   // the stream hub: Intra4x4 or Intra16x16 and the block modes of the marked macroblocks first, then the rows
        hipLaunchKernelGGL(k_i4_decide<true>, dim3(std::min((e->b_nmb + 3) / 4, (int)I4_MARKED_WAVES), pslots), dim3(64), 0, st, P, (int)G);
        hipLaunchKernelGGL((k_pintra_rows<false, true>), dim3(e->b_rows, pslots), dim3(64), 0, st, R);
    } else   // the encoder's own batches: ONE launch, the row waves decide as they go, and one load when the step has nothing for them
        hipLaunchKernelGGL((k_pintra_rows<false, false, true>), dim3(e->b_rows, pslots), dim3(64), 0, st, R);
}

// slice headers per position, from the pictures' records (Hpcm: of a picture with an I_PCM macroblock, which is not filtered)
void step_headers(mi355x_h264_encoder* e, const Step& T, HdrBatch& H, HdrBatch& Hpcm)
{
    for (int g = 0; g < T.n; g++) {
        const ItemPic& pic = T.items[g];
        uint64_t hdr = 0;
        H.len[g] = (unsigned char)build_slice_header(e->shape, T.idr, pic.idr_id, false, pic.frame_num, pic.qp, pic.nref, &hdr, pic.layer != 0);
        H.bits[g] = hdr;
        Hpcm.len[g] = (unsigned char)build_slice_header(e->shape, T.idr, pic.idr_id, true, pic.frame_num, pic.qp, pic.nref, &hdr, pic.layer != 0);
        Hpcm.bits[g] = hdr;
    }
}

// what the entropy coder's kernels and k_bs take
CavlcParams step_cavlc_params(mi355x_h264_encoder* e, const Step& T, const FrameParams& P)
{
    CavlcParams C{};
    C.mb = e->d_mb; C.levels = e->d_levels; C.mvd = e->d_mvd; C.mbw = e->mbw; C.nmb = e->nmb; C.p_slice = T.idr ? 0 : 1; C.t8x8 = e->cfg.profile_idc == 100 ? 1 : 0;
    C.nref = T.d_itemtab ? 0 : T.items[0].nref; C.sl = e->sl;   // (indirect launches: the position's own, from the itemtab word)
    C.mb_first = e->b_row0 * e->mbw; C.mb_end = C.mb_first + e->b_nmb;
    C.slice_cap = (unsigned)e->slice_cap;
    C.mbdiv = P.mbdiv;
    C.slotbits = e->d_slotbits; C.slotcode = e->d_slotcode; C.mbbits = e->d_mbbits; C.bitbuf = T.slot->d_bitbuf;
    C.bs = (uint8_t*)e->d_bs; C.prevcoded = e->d_prevcoded;
    C.st_mb = e->nmb; C.st_bitbuf = e->st_bitbuf_bytes / 4;
    C.aux = e->d_aux; C.mvq = e->d_mvq;
    C.src = T.d_src; C.w = e->cfg.width; C.h = e->cfg.height; C.src_nv12 = T.nv12 ? 1 : 0; C.st_src = T.src_item_stride;
    C.itemtab = T.d_itemtab; C.srctab = T.d_srctab;
    return C;
}

// the boundary strengths, a small launch in front of the fork (the diagonal debug form of the filter reads them too); returns the
// serial the loop filter of this picture will run under, 0 with the filter off
unsigned step_bs(mi355x_h264_encoder* e, const Step& T, const CavlcParams& C)
{
    if (e->cfg.disable_deblock) return 0;
    const unsigned db_serial = next_nonzero(e->serial);
    LAUNCH2(T.d_itemtab != nullptr, k_bs<true>, k_bs<false>, dim3(std::min((e->b_nmb + 1) / 2, (int)BS_WAVES), (unsigned)T.n), dim3(64), T.sync->st, C, e->d_anybs, db_serial);
    return db_serial;
}

// entropy coding on ec, k_mvpred through k_pack, and where the access units will lie (T.lay)
void step_entropy(mi355x_h264_encoder* e, Step& T, const FrameParams& P, const CavlcParams& C, const HdrBatch& H, const HdrBatch& Hpcm, hipStream_t ec)
{
    const bool idr = T.idr, ind = T.d_itemtab != nullptr;
    const unsigned G = (unsigned)T.n;
    Slot& S = *T.slot;
    StatScope sc(e, &S, MI355X_H264_K_CAVLC, 4, (uint32_t)(e->b_nmb * T.n), ec);
    const int grid = (e->b_nmb + 1) / 2;
    if (!idr) {
        LAUNCH2(ind, k_mvpred<true>, k_mvpred<false>, dim3((e->b_nmb + 63) / 64, G), dim3(64), ec, P);   // vectors + coded_block_pattern are final: mvd, P_Skip
        LAUNCH2(ind, k_skip_scan<true>, k_skip_scan<false>, dim3(G), dim3(256), ec, C);
    }
    LAUNCH2(ind, (k_cavlc<false, true>), (k_cavlc<false, false>), dim3(grid, G), dim3(64), ec, C);
    LAUNCH2(ind, k_bit_scan<true>, k_bit_scan<false>, dim3(G * (unsigned)e->b_nsl), dim3(SCAN_NT), ec, C, H, Hpcm, (const unsigned*)e->d_anypcm, P.pic_serial, S.d_info, e->d_me_cost,
            e->b_nsl, e->b_sl0, (unsigned)e->slice_cap);
    LAUNCH2(ind, (k_cavlc<true, true>), (k_cavlc<true, false>), dim3(grid, G), dim3(64), ec, C);
    // access unit layout in the pinned buffer: [pad][SPS PPS (IDR only)][00 00 00 01 hdr][payload...];
    // with several slices: the payload of slice s at s * slice_cap, the access unit is put together by finish_item
    const size_t pre = (idr ? e->sps_pps.size() : 0) + 5;
    const size_t pad = (16 - (pre & 15)) & 15;
    T.lay = AuLayout{pad, e->nsl > 1 ? 0 : pad + pre, idr};
    LAUNCH2(ind, k_pack<true>, k_pack<false>, dim3(G * (unsigned)e->b_nsl), dim3(SCAN_NT), ec, (uint8_t*)S.d_bitbuf, e->st_bitbuf_bytes, S.h_au + T.lay.payload_off, e->st_au,
            (const SliceInfo*)S.d_info, S.h_info, e->b_nsl, e->b_sl0, (unsigned)e->slice_cap, T.d_itemtab);
}

// debug (keep_pre): a copy of every picture's reconstruction before the loop filter
int step_keep_pre(mi355x_h264_encoder* e, const Step& T)
{
    hipStream_t st = T.sync->st;
    if (!T.d_itemtab && !T.inj)
        for (int p = 0; p < 3; p++) {   // (the items' planes lie nbuf ring slots apart: one row of the 2-D copy per item)
            const size_t ring = p ? e->st_ring_c : e->st_ring_y;
            HIPCHK(e->err, hipMemcpy2DAsync(e->d_pre[p], ring, e->d_planes[T.items[0].cur][p], p ? e->st_c : e->st_y, ring, (size_t)e->G, hipMemcpyDeviceToDevice, st));
        }
    if (T.d_itemtab)   // (mi355x_h264_stream_debug_keep_pre: every position's picture, from its item's own ring slot to its item's copy)
        for (int k = 0; k < T.n; k++)
            for (int p = 0; p < 3; p++) {
                const size_t ring = p ? e->st_ring_c : e->st_ring_y;
                HIPCHK(e->err, hipMemcpyAsync(e->d_pre[p] + (size_t)T.items[k].item * ring,
                                              e->d_plane_base[p] + (size_t)T.items[k].item * (p ? e->st_c : e->st_y) + (size_t)T.items[k].cur * ring, ring,
                                              hipMemcpyDeviceToDevice, st));
            }
    return MI355X_H264_OK;
}

// the loop filter, on the step's first stream
void step_filter(mi355x_h264_encoder* e, const Step& T, unsigned pic_serial, unsigned db_serial)
{
    const bool idr = T.idr, ind = T.d_itemtab != nullptr;
    const unsigned G = (unsigned)T.n;
    hipStream_t st = T.sync->st;
    const int steps = e->mbw + 2 * (e->mbh - 1);
    StatScope sc(e, T.slot, MI355X_H264_K_DEBLOCK, (uint32_t)(e->diag_mode ? steps : 1), (uint32_t)(e->b_nmb * T.n), st);
    const DbParams D = db_params(e, ind ? e->d_plane_base : e->d_planes[T.items[0].cur], e->sl, e->qp);   // (indirect launches look the item's own QP up on the device)
    if (e->diag_mode && !ind) {
        for (int s = 0; s < steps; s++) {
            const int ymin = std::max(0, (s - (e->mbw - 1) + 1) >> 1), ymax = std::min(e->mbh - 1, s >> 1);
            if (ymax < ymin) continue;
            hipLaunchKernelGGL(k_deblock_diag, dim3(ymax - ymin + 1), dim3(64), 0, st, D, s);
        }
        return;
    }
    DbRowParams R = db_row_params(e, D, T.sync->h_err, db_serial, pic_serial, e->b_row0, (int)G);
    R.itemtab = T.d_itemtab; R.st_ring_y = e->st_ring_y; R.st_ring_c = e->st_ring_c;
    // two macroblock rows per wave (k_deblock_pairs) for lockstep batches of pictures of one slice; else one row per wave
    const bool pairs = e->pair_filter && T.n >= e->pair_min_batch && e->nsl == 1 && e->b_rows == e->mbh;
    const unsigned grid_x = pairs ? (unsigned)((e->b_rows + 1) / 2) : (unsigned)e->b_rows;
    auto filter = [&](bool bs4, unsigned at_a_time) {   // (bs4 = false: the stream hub's P steps only)
        const dim3 grid(grid_x, std::min(G, at_a_time));
        if (pairs) { if (bs4) LAUNCH2(ind, (k_deblock_pairs<true, true>), (k_deblock_pairs<true, false>), grid, dim3(64), st, R);
                     else hipLaunchKernelGGL((k_deblock_pairs<false, true>), grid, dim3(64), 0, st, R); }
        else { if (bs4) LAUNCH2(ind, (k_deblock_rows<true, false, true>), (k_deblock_rows<true, false, false>), grid, dim3(64), st, R);
               else hipLaunchKernelGGL((k_deblock_rows<false, false, true>), grid, dim3(64), 0, st, R); }
    };
    if (idr) { R.need_intra = 0; filter(true, G); }
    else if (!ind) {   // P pictures: ONE launch, every picture resident and taken in the form it needs (k_deblock_rows_p)
        R.need_intra = 0;
        if (pairs) hipLaunchKernelGGL(k_deblock_pairs_p, dim3(grid_x, G), dim3(64), 0, st, R);
        else hipLaunchKernelGGL(k_deblock_rows_p, dim3(grid_x, G), dim3(64), 0, st, R);
    } else {   // P pictures of the stream hub: the form without the bS 4 filter, or - when the picture has intra macroblocks - the one with it
        // (while the recent P pictures had next to none, the second launch holds one picture at a time: see k_deblock_rows)
        R.need_intra = -1; filter(false, G);
        R.need_intra = 1; filter(true, e->p_intra_x16 > 16u * PINTRA_SPARSE_MBS ? G : 1u);
    }
}

// the quality report's comparisons on ec: k_sse, and k_ssim behind it on the same stream
void step_quality(mi355x_h264_encoder* e, const Step& T, const FrameParams& P, hipStream_t ec)
{
    const bool ind = T.d_itemtab != nullptr;
    const unsigned G = (unsigned)T.n;
    LAUNCH2(ind, k_sse<true>, k_sse<false>, dim3((unsigned)e->b_rows * SSE_SEGS, G), dim3(64), ec, P, T.slot->h_qpart, T.slot->h_qmap);
    if (T.lay.ssim) LAUNCH2(ind, k_ssim<true>, k_ssim<false>, dim3((unsigned)e->b_rows * SSIM_SEGS, G), dim3(64), ec, P, T.slot->h_spart, T.slot->h_smap);
}

// One lockstep step: the stages in order, and everything that orders the step's two streams - st carries reconstruction and loop
// filter (the chain to the next picture's motion search), ec entropy coding and the quality report beside them.
// (the payload buffers of the items were left zeroed by the k_pack of their previous use)
int submit_step(mi355x_h264_encoder* e, Step& T)
{
    const StepSync& Y = *T.sync;
    const bool ind = T.d_itemtab != nullptr;
    hipStream_t st = Y.st, ec = T.one_stream ? st : Y.ec;
    const bool fork = ec != st;
    const int cur = T.items[0].cur;   // (direct steps: the ring slot every item writes)
    FrameParams P;
    int me_pos[mi355x_h264_encoder::MAX_REFS] = {0, 0, 0};
    int rc = step_frame_params(e, T, P, me_pos);
    if (rc) return rc;
    // Quality report, hazard "ring slot": this picture's first kernels write ring slot `cur`, which the k_sse of the picture that
    // wrote it last read on the second stream - nbuf pictures ago, or, behind a layer-1 picture, the picture just before.  The event
    // is the slot's, so either way the wait below is the one that matters.  In mi355x_h264_encode_gops_device / _batch_device no host wait lies between the
    // two, so the rewrite is ordered behind that comparison by its event.  (Indirect steps: a stream's call returns only after the
    // host has waited for its step's `done`, which lies behind the step's k_sse - the host wait is the order.)
    if (!ind && e->q_done_set[cur]) {
        HIPCHK(e->err, hipStreamWaitEvent(st, e->q_done[cur], 0));
        e->q_done_set[cur] = false;
    }
    // reconstruction on st (or, mi355x_h264_debug_code_syntax, what it would have left)
    if (T.inj) { rc = step_inject(e, T, P); if (rc) return rc; }
    else if (T.idr) step_recon_idr(e, T, P);
    else step_recon_p(e, T, P, me_pos);
    HdrBatch H{}, Hpcm{};
    step_headers(e, T, H, Hpcm);
    const CavlcParams C = step_cavlc_params(e, T, P);
    const unsigned db_serial = step_bs(e, T, C);
    // entropy coding needs only levels / MbInfo, the loop filter the reconstruction and the boundary strengths: the two run side by
    // side and the filter never waits for the coder
    if (fork) {
        HIPCHK(e->err, hipEventRecord(Y.recon_ready, st));
        HIPCHK(e->err, hipStreamWaitEvent(ec, Y.recon_ready, 0));
    }
    step_entropy(e, T, P, C, H, Hpcm, ec);
    if (fork) HIPCHK(e->err, hipEventRecord(Y.entropy_done, ec));
    if (e->keep_pre) { rc = step_keep_pre(e, T); if (rc) return rc; }
    if (!e->cfg.disable_deblock && !T.inj) step_filter(e, T, P.pic_serial, db_serial);
    // Quality report: source against the reconstruction that is now final (behind the loop filter; behind the last reconstruction
    // kernel when nothing is filtered).  On the second stream, beside the entropy coder and behind the filter's event: the chain to the
    // next picture's k_me (this stream) does not wait for it.  An injected picture's ring holds nothing to compare.
    T.lay.quality = !e->quality_on ? 0 : (T.inj ? 2 : 1);
    T.lay.ssim = T.lay.quality && e->ssim_on;
    const bool compare = T.lay.quality == 1;
    if (compare) {
        if (fork) {
            HIPCHK(e->err, hipEventRecord(e->q_ready, st));
            HIPCHK(e->err, hipStreamWaitEvent(ec, e->q_ready, 0));
        }
        step_quality(e, T, P, ec);   // (k_ssim in front of q_done[cur] and `done` like k_sse: the three hazards hold for it unchanged)
        if (!ind) { HIPCHK(e->err, hipEventRecord(e->q_done[cur], ec)); e->q_done_set[cur] = true; }   // (hazard "ring slot", above)
    }
    if (fork) HIPCHK(e->err, hipStreamWaitEvent(st, Y.entropy_done, 0));   // join: the next picture rewrites MbInfo / levels
    // Hazard "source picture": a staging slot is handed to the next upload and a caller's device picture is valid only during the
    // call, and both happen after the host has waited for `done`.  With a comparison in the step `done` is therefore recorded on the
    // stream that runs it: that stream has waited for everything up to the filter on the other one and holds the entropy coder's
    // work itself, so the event lies behind the whole step and the host's one wait covers k_sse's loads and its stores to pinned memory.
    HIPCHK(e->err, hipEventRecord(Y.done, compare ? ec : st));
    HIPCHK(e->err, hipGetLastError());
    return MI355X_H264_OK;
}

// enqueue everything for one picture (every batch item's) whose I420 samples are at d_src: the direct form
int submit(mi355x_h264_encoder* e, const uint8_t* d_src, size_t src_item_stride, int slot_idx, bool nv12, const Injected* inj = nullptr)
{
    Slot& S = e->slots[slot_idx];
    // (after an injected picture, mi355x_h264_debug_code_syntax, nothing was reconstructed: a real picture has no reference then)
    const bool idr = e->seq.next_is_idr(e->cfg.gop) || (e->after_injected && !inj);
    e->seq.begin(idr);
    e->after_injected = inj != nullptr;
    for (int g = 0; g < e->G; g++) S.pics[g] = batch_item_pic(e->seq.pic(0, e->qp, idr, e->nrefs), g, e->idr_step);
    Step T;
    T.d_src = d_src; T.src_item_stride = src_item_stride; T.nv12 = nv12; T.idr = idr; T.n = e->G;
    T.items = S.pics;
    e->last_src = d_src;
    T.sync = &S.sync;
    T.slot = &S;
    T.inj = inj;
    const int rc = submit_step(e, T);
    if (rc) return rc;
    S.lay = T.lay;
    S.busy = true;
    e->seq.advance(idr, e->nbuf, e->idr_step * e->G);   // bookkeeping for the next picture
    return MI355X_H264_OK;
}

// wait for a slot (all batch items of one lockstep picture); stats are folded in once
int wait_slot(mi355x_h264_encoder* e, int slot_idx)
{
    Slot& S = e->slots[slot_idx];
    if (!S.busy) return set_err(e->err, MI355X_H264_E_INTERNAL, "collect on an idle slot");
    HIPCHK(e->err, hipEventSynchronize(S.sync.done));
    S.busy = false;
    for (auto& ev : S.evs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            e->stats.ms[ev.k] += ms; e->stats.launches[ev.k] += ev.launches; e->stats.mbs[ev.k] += ev.mbs;
        }
        e->ev_pool.push_back(ev.a); e->ev_pool.push_back(ev.b);
    }
    S.evs.clear();
    e->stats.frames += (uint64_t)e->G;
    const int rc = handoff_timeout(S.sync, e->err);
    if (rc) e->seq.force_idr = 1;   // the picture's reconstruction is not to be trusted: it must not become a reference
    return rc;
}

// finish the access unit of picture `pic` on the host: S = the buffers it was written to, L = where and of which type
int finish_au(mi355x_h264_encoder* e, Slot& S, const AuLayout& L, const ItemPic& pic, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    const int g = pic.item, nal_hdr = slice_nal_hdr(L.idr, pic.layer);
    uint8_t* base = S.h_au + (size_t)g * e->st_au;
    const SliceInfo* const info = S.h_info + (size_t)g * e->b_nsl;   // one per slice of this instance's band
    for (int sl = 0; sl < e->b_nsl; sl++)
        if (info[sl].error) {
            e->seq.force_idr = 1;   // the refused picture is missing from the stream: the next one must not refer to it
            const int code = info[sl].error == 1 ? MI355X_H264_E_OVERFLOW : MI355X_H264_E_INTERNAL;
            if (e->nsl > 1) return set_err(e->err, code, "device reported error %u (slice %d)", info[sl].error, sl);
            return set_err(e->err, code, "device reported error %u", info[sl].error);
        }
    // what the picture tells the statistics, the scene-change measure and the sizing of the next P pictures' intra pass
    uint32_t cost = 0, searched = 0, tq_coded = 0;
    size_t need = e->sps_pps.size() + 16;
    for (int sl = 0; sl < e->b_nsl; sl++) {
        cost += info[sl].me_cost; searched += info[sl].searched; tq_coded += info[sl].tq_coded;
        need += 5 + (size_t)info[sl].total_bytes * 3 / 2 + 16;
    }
    e->last_me_cost[g] = cost;
    if (!L.idr) {
        e->stats.p_mbs += (uint64_t)e->b_nmb; e->stats.me_searched_mbs += searched; e->stats.tq_coded_mbs += tq_coded;
        e->p_intra_x16 = (3 * e->p_intra_x16 + 16 * (searched - tq_coded)) / 4;
    }
    if (frame_type) *frame_type = L.idr ? MI355X_H264_FRAME_IDR : MI355X_H264_FRAME_P;
    e->last_layer = pic.layer;
    e->last_rband[g] = pic.rband;
    std::vector<uint8_t>& eb = e->esc_buf[g];
    if (e->nsl > 1) {
        // several slices: one NAL unit each, put together here (the payloads lie slice_cap apart in the pinned buffer)
        size_t pos = 0;
        if (pic.rband == 0) {   // intra refresh: the access unit that starts a cycle opens with the recovery point SEI
            eb.clear();
            append_recovery_point_sei(eb, e->nsl);   // (n = the stream's slices)
            pos = eb.size();
        }
        eb.resize(need + pos);
        if (L.idr && e->b_sl0 == 0) { memcpy(eb.data(), e->sps_pps.data(), e->sps_pps.size()); pos = e->sps_pps.size(); }   // parameter sets go with the first band
        for (int sl = 0; sl < e->b_nsl; sl++) {
            const SliceInfo& si = info[sl];
            const uint8_t* pay = base + (size_t)(e->b_sl0 + sl) * e->slice_cap;
            uint8_t* o = eb.data() + pos;
            o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 1; o[4] = (uint8_t)nal_hdr;
            pos += 5;
            if (si.epb_count == 0) { memcpy(eb.data() + pos, pay, si.total_bytes); pos += si.total_bytes; }
            else pos += nal_escape(pay, si.total_bytes, eb.data() + pos);
        }
        *out = eb.data();
        *out_len = (uint32_t)pos;
        return MI355X_H264_OK;
    }
    // one slice: the kernels wrote the payload behind the room left for parameter sets and NAL header
    uint8_t* au = base + L.au_start;
    size_t pos = 0;
    if (L.idr) { memcpy(au, e->sps_pps.data(), e->sps_pps.size()); pos = e->sps_pps.size(); }
    au[pos++] = 0; au[pos++] = 0; au[pos++] = 0; au[pos++] = 1; au[pos++] = (uint8_t)nal_hdr;
    if (info->epb_count == 0) {
        *out = au;
        *out_len = (uint32_t)(pos + info->total_bytes);
    } else {  // rare: some 00 00 0x pattern needs an emulation prevention byte
        eb.resize(pos + (size_t)info->total_bytes * 3 / 2 + 16);
        memcpy(eb.data(), au, pos);
        const size_t n = nal_escape(base + L.payload_off, info->total_bytes, eb.data() + pos);
        *out = eb.data();
        *out_len = (uint32_t)(pos + n);
    }
    return MI355X_H264_OK;
}

// the quality record of picture `pic`: the rows of the band added up (k_sse left one partial per wave and plane).  A
// picture that was refused (E_OVERFLOW) or injected has a record with valid = 0
void quality_record(mi355x_h264_encoder* e, const Slot& S, const AuLayout& L, const ItemPic& pic, uint32_t bytes, bool compared)
{
    const int g = pic.item;
    mi355x_h264_quality q{};
    q.bytes = bytes; q.qp = (uint32_t)pic.qp; q.frame_type = L.idr ? MI355X_H264_FRAME_IDR : MI355X_H264_FRAME_P;
    e->q_map[g] = nullptr;
    if (compared) {
        const unsigned long long* part = S.h_qpart + ((size_t)g * e->mbh + e->b_row0) * SSE_SEGS * 3;
        for (int r = 0; r < e->b_rows * SSE_SEGS; r++)
            for (int p = 0; p < 3; p++) q.sse[p] += part[(size_t)r * 3 + p];
        // display samples of the band's rows
        const int w = e->cfg.width, h = e->cfg.height;
        const int y0 = std::min(h, 16 * e->b_row0), y1 = std::min(h, 16 * (e->b_row0 + e->b_rows));
        const int c0 = std::min(h / 2, 8 * e->b_row0), c1 = std::min(h / 2, 8 * (e->b_row0 + e->b_rows));
        q.samples[0] = (uint64_t)(y1 - y0) * w;
        q.samples[1] = q.samples[2] = (uint64_t)(c1 - c0) * (w / 2);
        q.valid = 1;
        e->q_map[g] = S.h_qmap + (size_t)g * e->nmb;
    }
    e->q_item[g] = q;
    e->q_have[g] = 1;
    const size_t idx = (size_t)g * e->q_mul + e->q_add;
    if (idx < e->q_recs.size()) e->q_recs[idx] = q;
    if (!e->ssim_ready) return;
    // the SSIM record beside it (k_ssim left one partial per wave and plane; the window counts follow from the geometry)
    e->s_map[g] = nullptr;
    e->s_have[g] = 0;
    if (!L.ssim) return;
    mi355x_h264_ssim s{};
    if (compared) {
        const long long* part = S.h_spart + ((size_t)g * e->mbh + e->b_row0) * SSIM_SEGS * 3;
        for (int r = 0; r < e->b_rows * SSIM_SEGS; r++)
            for (int p = 0; p < 3; p++) s.sum[p] += part[(size_t)r * 3 + p];
        // windows at (4i, 4j) that lie wholly inside the display samples of the band's rows
        const int w = e->cfg.width, h = e->cfg.height;
        const int yl = std::min(h, 16 * (e->b_row0 + e->b_rows)) - 16 * e->b_row0, cl = std::min(h / 2, 8 * (e->b_row0 + e->b_rows)) - 8 * e->b_row0;
        auto count = [](int span) { return (uint64_t)std::max(0, span / 4 - 1); };
        s.windows[0] = count(w) * count(yl);
        s.windows[1] = s.windows[2] = count(w / 2) * count(cl);
        s.valid = 1;
        e->s_map[g] = S.h_smap + (size_t)g * e->nmb;
    }
    e->s_item[g] = s;
    e->s_have[g] = 1;
    if (idx < e->s_recs.size()) e->s_recs[idx] = s;
}

int finish_item(mi355x_h264_encoder* e, Slot& S, const AuLayout& L, const ItemPic& pic, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    const int rc = finish_au(e, S, L, pic, out, out_len, frame_type);
    const int g = pic.item;
    if (L.quality) quality_record(e, S, L, pic, rc == MI355X_H264_OK ? *out_len : 0, rc == MI355X_H264_OK && L.quality == 1);
    else {   // (coded with the switch off: nothing to read for this picture)
        if (!e->q_have.empty()) e->q_have[g] = 0;
        if (!e->s_have.empty()) e->s_have[g] = 0;
    }
    return rc;
}

// a call begins: room for the records of its n pictures (none while the switch is off); item g's record goes to g * mul + add
void quality_begin(mi355x_h264_encoder* e, size_t n, size_t mul, size_t add)
{
    e->q_recs.clear();
    if (e->quality_on) e->q_recs.resize(n);   // (valid = 0 until the picture is finished)
    e->s_recs.clear();
    if (e->quality_on && e->ssim_on) e->s_recs.resize(n);
    e->q_mul = mul; e->q_add = add;
}

// the switch of the quality report; the pinned result arrays of every slot and the events come with the first enable
hipError_t quality_alloc(mi355x_h264_encoder* e)
{
    if (e->q_ready) return hipSuccess;
    HIPTRY(hipSetDevice(e->device));
    const size_t Gn = (size_t)e->G, part = Gn * e->mbh * SSE_SEGS * 3 * sizeof(unsigned long long), map = Gn * e->nmb * sizeof(uint32_t);
    for (int si = 0; si < e->nslots; si++) {
        Slot& S = e->slots[si];
        HIPTRY(DM_PINNED(e->mem, S.h_qpart, part));
        HIPTRY(DM_PINNED(e->mem, S.h_qmap, map));
        memset(S.h_qpart, 0, part);
        memset(S.h_qmap, 0, map);   // (a band instance's kernel stores its own rows only: the others stay 0)
    }
    for (int b = 0; b < e->nbuf; b++) HIPTRY(hipEventCreateWithFlags(&e->q_done[b], hipEventDisableTiming));
    e->q_item.assign(Gn, mi355x_h264_quality{});
    e->q_map.assign(Gn, nullptr);
    e->q_have.assign(Gn, 0);
    HIPTRY(hipEventCreateWithFlags(&e->q_ready, hipEventDisableTiming));
    return hipSuccess;
}
// k_ssim's pinned result arrays, in every slot: with the first enable that asks for SSIM
hipError_t ssim_alloc(mi355x_h264_encoder* e)
{
    if (e->ssim_ready) return hipSuccess;
    HIPTRY(hipSetDevice(e->device));
    const size_t Gn = (size_t)e->G, part = Gn * e->mbh * SSIM_SEGS * 3 * sizeof(long long), map = Gn * e->nmb * sizeof(int32_t);
    for (int si = 0; si < e->nslots; si++) {
        Slot& S = e->slots[si];
        if (!S.h_spart) { HIPTRY(DM_PINNED(e->mem, S.h_spart, part)); memset(S.h_spart, 0, part); }
        if (!S.h_smap) { HIPTRY(DM_PINNED(e->mem, S.h_smap, map)); memset(S.h_smap, 0, map); }   // (rows outside the band stay 0)
    }
    e->s_item.assign(Gn, mi355x_h264_ssim{});
    e->s_map.assign(Gn, nullptr);
    e->s_have.assign(Gn, 0);
    e->ssim_ready = true;
    return hipSuccess;
}
// metrics: MI355X_H264_QUALITY_* bits; 0 off, SSE alone, or both (SSIM alone is refused: its record accompanies the SSE record)
int quality_set(mi355x_h264_encoder* e, unsigned metrics)
{
    if (!quality_metrics_ok(metrics))
        return set_err(e->err, MI355X_H264_E_ARG, "quality report: metrics must be 0, MI355X_H264_QUALITY_SSE, or SSE | SSIM (the SSIM record accompanies the SSE record)");
    if (metrics) {
        hipError_t r = quality_alloc(e);
        if (r == hipSuccess && (metrics & MI355X_H264_QUALITY_SSIM)) r = ssim_alloc(e);
        if (r != hipSuccess) return set_err(e->err, r == hipErrorOutOfMemory ? MI355X_H264_E_NOMEM : MI355X_H264_E_HIP, "quality report: %s: %s", t_failed_call, hipGetErrorString(r));
    }
    e->quality_on = metrics != 0;
    e->ssim_on = (metrics & MI355X_H264_QUALITY_SSIM) != 0;
    return MI355X_H264_OK;
}

int collect(mi355x_h264_encoder* e, int slot_idx, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    const int rc = wait_slot(e, slot_idx);
    return rc ? rc : finish_item(e, e->slots[slot_idx], e->slots[slot_idx].lay, e->slots[slot_idx].pics[0], out, out_len, frame_type);
}

void destroy_engine(mi355x_h264_encoder* e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->stream_ec && e->stream_ec != e->stream) (void)hipStreamSynchronize(e->stream_ec);
    pic_store_destroy(*e);   // (its list holds the engine's own allocations too)
    for (auto& S : e->slots) {
        sync_destroy(S.sync);
        for (auto& ev : S.evs) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
    }
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->q_done) if (ev) (void)hipEventDestroy(ev);
    if (e->q_ready) (void)hipEventDestroy(e->q_ready);
    if (e->stream_ec && e->stream_ec != e->stream) (void)hipStreamDestroy(e->stream_ec);
    if (e->counted_live) e->counted_live->fetch_sub(1);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// the store, then what is the encoder's alone: streams, device and pinned memory of a configured engine
hipError_t engine_alloc(mi355x_h264_encoder* e, bool hub_engine)
{
    DevMem& M = e->mem;
    M.configure();   // the guard mode of dev_mem.h, as the process-wide switch stands now
    HIPTRY(pic_store_create(*e, e->device, e->mbw, e->mbh, e->G, e->nbuf));
    HIPTRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    // Entropy coding normally runs on a stream of its own beside the loop filter (shorter picture latency).  A process that
    // holds many engines (the plugin surface with many streams: one engine per VideoEncoder object) would then ask for more
    // hardware queues than the device has, and the runtime's multiplexing costs more than the overlap gains (16 plugin streams: 3.8 k -> 6.0 k fps; 4 streams: p99 8 -> 4 ms): from the third
    // live engine on (or with MI355X_H264_ONE_STREAM=1) an engine uses its one stream for everything.
    {
        static std::atomic<int> live{0};
        const char* one = getenv("MI355X_H264_ONE_STREAM");
        const int n = live.fetch_add(1) + 1;
        e->counted_live = &live;
        if ((one && one[0] == '1') || (n > 2 && !(one && one[0] == '0'))) e->stream_ec = e->stream;
        else HIPTRY(hipStreamCreateWithFlags(&e->stream_ec, hipStreamNonBlocking));
    }
    const size_t ysz = (size_t)e->cw * e->ch;
    const size_t Gn = (size_t)e->G, nmb = Gn * e->nmb;   // (nmb: macroblocks of all batch items)
    static const char* const pre_name[3] = {"d_pre[0]", "d_pre[1]", "d_pre[2]"};
    for (int p = 0; p < 3; p++) HIPTRY(M.dev(&e->d_pre[p], (p ? e->st_ring_c : e->st_ring_y) * Gn, false, pre_name[p]));
    {
        std::vector<QpEntry> qt(52);
        for (int q = 0; q < 52; q++) fill_qp(qt[q].qy, qt[q].qc, qt[q].lambda, qt[q].sad_nz, q);
        HIPTRY(DM_DEV(M, e->d_qtab, 52 * sizeof(QpEntry), false));
        HIPTRY(hipMemcpy(e->d_qtab, qt.data(), 52 * sizeof(QpEntry), hipMemcpyHostToDevice));
    }
    HIPTRY(DM_DEV(M, e->d_mvd, nmb * 8 * sizeof(int16_t), false));
    HIPTRY(DM_DEV(M, e->d_me_total, nmb * sizeof(uint32_t), false));
    HIPTRY(DM_DEV(M, e->d_pmv, nmb * sizeof(int), false));
    HIPTRY(DM_DEV(M, e->d_slotbits, nmb * 32 * sizeof(uint16_t), false));
    HIPTRY(DM_DEV(M, e->d_slotcode, nmb * 32 * sizeof(unsigned long long), false));
    HIPTRY(DM_DEV(M, e->d_mbbits, nmb * sizeof(uint32_t), false));
    HIPTRY(DM_DEV(M, e->d_prevcoded, Gn * (e->nmb + 1) * sizeof(int32_t), false));
    HIPTRY(DM_DEV(M, e->d_me_cost, nmb * sizeof(uint16_t), true));
    e->frame_bytes = (size_t)e->cfg.width * e->cfg.height * 3 / 2;
    HIPTRY(DM_DEV(M, e->d_stage, e->frame_bytes + 256, false));
    HIPTRY(DM_PINNED(M, e->h_stage, e->frame_bytes + 256));
    e->bitbuf_cap = ysz * 2 + (1 << 16);
    e->slice_cap = e->bitbuf_cap;
    if (e->nsl > 1) {   // every slice gets room for twice its luma bytes (CAVLC's worst case is about 1.6 times)
        e->slice_cap = ((size_t)e->sl.rows * 256 * e->mbw * 2 + 4096 + 15) & ~(size_t)15;
        e->bitbuf_cap = e->slice_cap * e->nsl;
    }
    e->st_bitbuf_bytes = (e->bitbuf_cap + 256 + 255) & ~(size_t)255;
    e->au_cap = e->bitbuf_cap + e->sps_pps.size() + 64;
    e->st_au = (e->au_cap + 256 + 255) & ~(size_t)255;
    e->nslots = hub_engine ? 1 : NSLOT;
    if (!hub_engine && e->G >= TURN_MIN_BATCH && e->device >= 0 && e->device < TURN_DEVICES) {   // takes part in the turn-taking of the motion searches
        std::lock_guard<std::mutex> tl(g_turns.mu);
        if (!g_turns.d_lock[e->device]) {
            HIPTRY(hipMalloc((void**)&g_turns.d_lock[e->device], sizeof(unsigned)));
            HIPTRY(hipMemset(g_turns.d_lock[e->device], 0, sizeof(unsigned)));
        }
        e->me_turn = (int)g_turns.next_id++;
    }
    for (int si = 0; si < e->nslots; si++) {
        Slot& S = e->slots[si];
        HIPTRY(DM_DEV(M, S.d_bitbuf, e->st_bitbuf_bytes * Gn, true));
        HIPTRY(DM_DEV(M, S.d_info, sizeof(SliceInfo) * Gn * e->nsl, false));
        HIPTRY(DM_PINNED(M, S.h_info, sizeof(SliceInfo) * Gn * e->nsl));
        HIPTRY(DM_PINNED(M, S.h_au, e->st_au * Gn));
        HIPTRY(sync_create(S.sync, e->stream, e->stream_ec, false));
    }
    HIPTRY(hipDeviceSynchronize());
    return hipSuccess;
}

// hub_engine: the engine of a stream hub (hub.h) - one set of output buffers instead of NSLOT, never more than one HIP stream
// pair of its own (the hub's step contexts bring theirs)
// colour: the stream's description (null: none); chroma_loc: its VUI says where the chroma samples lie (a hub of RGBA input)
int create_engine(const mi355x_h264_config* cfg, mi355x_h264_encoder** out, bool hub_engine, const ColourDesc* colour = nullptr, bool chroma_loc = false)
{
    if (!cfg || !out || cfg->struct_size != sizeof(mi355x_h264_config)) return MI355X_H264_E_ARG;
    if (colour && colour->described && !colour_valid(colour->matrix, colour->full_range)) return MI355X_H264_E_ARG;
    ask_for_hw_queues();   // (here, not only in the store's create: the device count below brings the runtime up)
    *out = nullptr;
    if (cfg->width < 16 || cfg->height < 16 || cfg->width > 4096 || cfg->height > 4096 || ((cfg->width | cfg->height) & 1) ||
        cfg->qp < 10 || cfg->qp > 51 || cfg->gop < 1 || (cfg->profile_idc != 66 && cfg->profile_idc != 77 && cfg->profile_idc != 100) ||
        (cfg->input_format != MI355X_H264_INPUT_I420 && cfg->input_format != MI355X_H264_INPUT_NV12) || cfg->slices < 0 || cfg->slices > 64 ||
        cfg->refs < 0 || cfg->refs > mi355x_h264_encoder::MAX_REFS || (cfg->search != MI355X_H264_SEARCH_EXHAUSTIVE && cfg->search != MI355X_H264_SEARCH_SEEDED))
        return MI355X_H264_E_ARG;
    if (cfg->band_count < 0 || cfg->band_index < 0 || (cfg->band_count > 1 && (cfg->band_index >= cfg->band_count || cfg->batch > 1))) return MI355X_H264_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return MI355X_H264_E_NODEVICE;
    mi355x_h264_encoder* e = new (std::nothrow) mi355x_h264_encoder();
    if (!e) return MI355X_H264_E_NOMEM;
    e->cfg = *cfg;
    e->device = cfg->device;
    e->qp = cfg->qp;
    e->mbw = (cfg->width + 15) / 16; e->mbh = (cfg->height + 15) / 16;
    e->cw = e->mbw * 16; e->ch = e->mbh * 16; e->nmb = e->mbw * e->mbh;
    e->level_idc = std::max(32, pick_level(e->nmb, cfg->fps > 0 ? cfg->fps : 30));
    {   // slices: bands of ceil(rows / slices) macroblock rows, at least two rows each
        const int n = std::min(std::max(cfg->slices, 1), std::max(1, e->mbh / 2));
        e->sl.rows = (e->mbh + n - 1) / n;
        e->sl.inv = recip32(e->sl.rows);   // (one row: my is always 0)
        e->nsl = (e->mbh + e->sl.rows - 1) / e->sl.rows;
    }
    e->b_sl0 = 0; e->b_nsl = e->nsl;
    if (cfg->band_count > 1) {   // this instance codes its share of the slices; the others belong to the neighbours
        if (cfg->band_count > e->nsl) { delete e; return MI355X_H264_E_ARG; }
        e->b_sl0 = (int)((long)cfg->band_index * e->nsl / cfg->band_count);
        e->b_nsl = (int)((long)(cfg->band_index + 1) * e->nsl / cfg->band_count) - e->b_sl0;
    }
    e->b_row0 = e->b_sl0 * e->sl.rows;
    e->b_rows = std::min(e->mbh, (e->b_sl0 + e->b_nsl) * e->sl.rows) - e->b_row0;
    e->b_nmb = e->b_rows * e->mbw;
    e->nrefs = cfg->refs > 1 ? cfg->refs : 1;
    e->nbuf = e->nrefs + 1;
    e->G = cfg->batch > 1 ? cfg->batch : 1;
    if (e->G > MAX_BATCH) { delete e; return MI355X_H264_E_ARG; }
    e->esc_buf.resize((size_t)e->G);
    e->last_me_cost.assign((size_t)e->G, 0);
    e->last_rband.assign((size_t)e->G, -1);
    if (colour) e->colour = *colour;
    e->shape = StreamShape{cfg->profile_idc, e->level_idc, e->nrefs, e->mbw, e->mbh, cfg->width, cfg->height, e->nsl, cfg->disable_deblock,
                           e->colour.described, e->colour.matrix, e->colour.full_range, chroma_loc ? 1 : 0, cfg->fps > 0 ? cfg->fps : 30, 0};
    e->sps_pps = build_parameter_sets(e->shape);
    e->diag_mode = getenv("MI355X_H264_DIAG") != nullptr && e->G == 1 && e->b_nsl == e->nsl;
    {
        // The loop filter takes two macroblock rows per wave (k_deblock_pairs) from a lockstep batch of 8 pictures on (pictures of one
        // slice): measured on the bench workload with the filter's edge skip in place, same box, row form / pair form: batch 4
        // 8 837 / 8 851 fps, batch 8 15.0 / 15.3 k, batch 16 21.2 / 22.1 k, batch 32 24.0 / 25.0 k; one GOP in flight 1 230 / 1 209 fps -
        // so small batches and the latency mode keep one row per wave.  MI355X_H264_PAIR_FILTER=N moves the threshold, 0 turns the
        // pair form off.
        const char* pf = getenv("MI355X_H264_PAIR_FILTER");
        e->pair_filter = !(pf && pf[0] == '0');
        e->pair_min_batch = (pf && pf[0] >= '1' && pf[0] <= '9') ? atoi(pf) : 8;
    }
    const hipError_t r = engine_alloc(e, hub_engine);
    if (r != hipSuccess) {
        fprintf(stderr, "mi355x_h264_create: %s: %s\n", t_failed_call, hipGetErrorString(r));
        destroy_engine(e);
        return r == hipErrorOutOfMemory ? MI355X_H264_E_NOMEM : MI355X_H264_E_HIP;
    }
    {   // MI355X_H264_QUALITY=1: the quality report is on from the first picture (mi355x_h264_quality_enable); =3: with SSIM (_enable_ex)
        const unsigned metrics = quality_env_metrics(getenv("MI355X_H264_QUALITY"));
        if (metrics && quality_set(e, metrics) != MI355X_H264_OK) {
            fprintf(stderr, "mi355x_h264_create: %s\n", e->err);
            destroy_engine(e);
            return MI355X_H264_E_HIP;
        }
    }
    *out = e;
    return MI355X_H264_OK;
}

int take_slot(mi355x_h264_encoder* e) { const int slot = e->next_slot; e->next_slot = (slot + 1) % NSLOT; return slot; }

// one picture already in device memory, in the given layout
int encode_one_device(mi355x_h264_encoder* e, const void* d_pic, bool nv12, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    HIPCHK(e->err, hipSetDevice(e->device));
    const int slot = take_slot(e);
    if (e->G != 1) return set_err(e->err, MI355X_H264_E_ARG, "single-picture calls need a batch-1 encoder");
    quality_begin(e, 1, 1, 0);
    int rc = submit(e, (const uint8_t*)d_pic, 0, slot, nv12);
    if (rc) return rc;
    return collect(e, slot, out, out_len, frame_type);
}

// A host picture on its way to the device: tight in pinned memory (h_dst), then the transfer to d_dst on st.  A picture that is
// tight where it lies (the reference's own layout, InitSrcPic ref :354-365: no per-row work) goes in `pieces` pieces, the copy
// of piece k + 1 overlapping the transfer of piece k; any other in one transfer.
hipError_t stage_picture(const HostPicture& in, int w, int h, uint8_t* h_dst, uint8_t* d_dst, hipStream_t st, int pieces)
{
    const size_t n = picture_bytes(in.layout, w, h);
    if (!picture_is_tight(in, w, h)) {
        pack_picture(in, w, h, h_dst);
        return hipMemcpyAsync(d_dst, h_dst, n, hipMemcpyHostToDevice, st);
    }
    const size_t piece = pieces > 1 ? ((n / pieces) + 255) & ~(size_t)255 : n;
    for (size_t o = 0; o < n; o += piece) {
        const size_t len = std::min(piece, n - o);
        memcpy(h_dst + o, in.p[0] + o, len);
        HIPTRY(hipMemcpyAsync(d_dst + o, h_dst + o, len, hipMemcpyHostToDevice, st));
    }
    return hipSuccess;
}

// a host I420 / NV12 picture through the engine's staging pair (the previous picture's use of it has completed: encode is synchronous)
int encode_one_host(mi355x_h264_encoder* e, const HostPicture& in, int pieces, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    HIPCHK(e->err, hipSetDevice(e->device));
    HIPCHK(e->err, stage_picture(in, e->cfg.width, e->cfg.height, e->h_stage, e->d_stage, e->stream, pieces));
    return encode_one_device(e, e->d_stage, in.layout == PIC_NV12, out, out_len, frame_type);
}

// an RGBA picture in device memory: one conversion pass into the I420 staging picture
int encode_rgba_from_device(mi355x_h264_encoder* e, const uint8_t* d_rgba, size_t stride, uint8_t** out, uint32_t* out_len, int* frame_type)
{
    const int w = e->cfg.width, h = e->cfg.height;
    launch_rgba_to_i420(e->colour.described ? colour_variant(e->colour.matrix, e->colour.full_range) : 0, dim3((unsigned)((w / 2 + 255) / 256), (unsigned)(h / 2)), e->stream, d_rgba, stride, e->d_stage, w, h);
    HIPCHK(e->err, hipGetLastError());
    return encode_one_device(e, e->d_stage, false, out, out_len, frame_type);
}

// `count` lockstep pictures with NSLOT - 1 of them in flight: submit_pic(i, slot) queues picture i, consume(i, slot) waits for
// the slot and takes what it holds.  On an error the pictures still in flight are waited for (and dropped) before returning -
// no slot stays busy - and the first error's text stays.
template <class SubmitPic, class Consume>
int run_pipeline(mi355x_h264_encoder* e, int count, SubmitPic&& submit_pic, Consume&& consume)
{
    int pending[NSLOT], npend = 0, head = 0;
    auto drain_one = [&]() -> int { const int rc = consume(head, pending[head % NSLOT]); if (rc == 0) { head++; npend--; } return rc; };
    auto bail = [&](int rc) -> int {
        char first[sizeof(e->err)];
        memcpy(first, e->err, sizeof(first));
        for (; npend > 0; head++, npend--) (void)wait_slot(e, pending[head % NSLOT]);   // (an idle slot says so and is passed over)
        memcpy(e->err, first, sizeof(first));
        return rc;
    };
    for (int i = 0; i < count; i++) {
        if (npend == NSLOT - 1) { int rc = drain_one(); if (rc) return bail(rc); }
        pending[i % NSLOT] = take_slot(e);
        int rc = submit_pic(i, pending[i % NSLOT]);
        if (rc) return bail(rc);
        npend++;
    }
    while (npend) { int rc = drain_one(); if (rc) return bail(rc); }
    return MI355X_H264_OK;
}

// ---- slice bands over several GPUs: the rows next to a band in the reference picture come from the neighbours ----
enum { HALO_MB_ROWS = 2 };   // 32 luma rows: the search reaches 16 rows + 0.75 + the 6-tap filter's 3, chroma half of that
// rows [r0, r1) of the newest reconstruction <-> a packed block (Y rows, then U rows, then V rows)
int halo_copy(mi355x_h264_encoder* e, int r0, int r1, void* d_blk, bool to_block)
{
    const int last = e->seq.last_slot(e->nbuf);
    uint8_t* blk = (uint8_t*)d_blk;
    for (int p = 0; p < 3; p++) {
        const size_t pitch = p ? e->cw / 2 : e->cw, rows_per_mb = p ? 8 : 16;
        const size_t off = (size_t)r0 * rows_per_mb * pitch, n = (size_t)(r1 - r0) * rows_per_mb * pitch;
        uint8_t* pl = e->d_planes[last][p] + off;
        if (n) HIPCHK(e->err, hipMemcpyAsync(to_block ? (void*)blk : (void*)pl, to_block ? (const void*)pl : (const void*)blk, n, hipMemcpyDefault, e->stream));   // the block may be device or host memory
        blk += (size_t)HALO_MB_ROWS * rows_per_mb * pitch;   // fixed layout, whatever the number of rows present
    }
    HIPCHK(e->err, hipStreamSynchronize(e->stream));
    return MI355X_H264_OK;
}

}  // namespace
