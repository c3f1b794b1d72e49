// media_amd/csrc/hub_sched.h -- the stream hub's scheduling, without HIP (hub.h brings uploads and the step as callables;
// tools/hub_sched_harness.cpp drives this file alone under ThreadSanitizer).  No thread is created: the caller that finds a free
// step context becomes the step's leader (gathers what is queued, runs the step, marks its pictures done), the others sleep until
// their picture is done.  P and IDR pictures never share a step: an IDR picture's row wavefront runs for milliseconds.  Contexts
// 0 .. nctx_p - 1 take the P steps (one's loop filter overlaps the other's motion search), context nctx_p the IDR steps.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

#include "host_framing.h"   // PicSeq, ItemPic

namespace {

enum { HUB_MAX_ITEMS = 64, HUB_MAX_CTX = 9 };

inline uint64_t now_us() { return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#ifndef HUB_SCHED_CLOCK   // (the clock of the gather window's deadline; the sanitizer harness has to take another)
#define HUB_SCHED_CLOCK std::chrono::steady_clock
#endif

// a gathered step: picks[k] = the stream (batch item) and what its slice header and the kernels need, as they stood when the step
// was gathered with nopen streams open, ordered by the pictures' number of reference pictures (most first); rc[k] is the step runner's answer for it (0: the picture is in the stream)
struct HubStep { int ctx; bool idr; int n, nopen; ItemPic picks[HUB_MAX_ITEMS]; int rc[HUB_MAX_ITEMS]; };

struct HubSched {
    std::mutex mu;                   // everything below
    std::condition_variable cv;
    int cap = 0, nopen = 0, uploading = 0;
    int nctx_p = 2;                  // contexts for P steps
    int window_us = 200;             // how long a P step that is being gathered waits for pictures still being uploaded
    int nrefs = 1;                   // reference pictures every stream of the hub searches (config.refs)
    int nbuf = 2;                    // reconstruction ring slots per stream: nrefs + 1
    bool collecting = false;         // a leader is gathering a P step
    bool busy[HUB_MAX_CTX] = {};
    std::vector<int> queue[2];       // [0] P pictures, [1] IDR pictures waiting for a step
    struct Item {
        bool open = false, done = false;
        PicSeq seq;                  // coding state of the stream (what the engine keeps for its one stream)
        int qp = 26, gop = 30;
        int last_cur = 0;            // ring slot of the last finished picture
        int last_layer = 0;          // and its temporal layer
        int last_rband = -1;         // and its all-intra band (intra refresh; -1: an IDR picture, or refresh off)
        uint64_t step_serial = 0;    // the step that took the stream's last picture: its number on this hub (1, 2, ..), how many
        int step_n = 0, step_pos = 0;   // pictures it carried, this picture's position in it, and its type (test hook:
        bool step_idr = false;       // mi355x_h264_stream_debug_last_step)
    } items[HUB_MAX_ITEMS];
    uint64_t steps = 0, pictures = 0, max_batch = 0;
    std::atomic<uint64_t> us_queue{0};

    bool any_busy() const { for (int i = 0; i <= nctx_p; i++) if (busy[i]) return true; return false; }
    // A P step takes at most its share of the open streams: with nctx_p steps in flight and one share uploading, a context
    // that frees finds pictures already uploaded instead of waiting for the streams it has just released to come back
    size_t p_share() const { return std::max<size_t>(1, ((size_t)nopen + nctx_p) / (nctx_p + 1)); }

    bool has_room() { std::lock_guard<std::mutex> lk(mu); return nopen < cap; }
    int open(int qp, int gop, int layers = 1, int refresh_n = 0)   // refresh_n: bands of an intra refresh stream, 0 = an ordinary one
    {
        std::lock_guard<std::mutex> lk(mu);
        int idx = 0;
        while (idx < cap && items[idx].open) idx++;
        if (idx >= cap) return -1;
        items[idx] = Item();
        items[idx].open = true; items[idx].qp = qp; items[idx].gop = gop; items[idx].seq.layers = layers;
        items[idx].seq.refresh_n = refresh_n;
        nopen++;
        return idx;
    }
    // true: that was the last open stream, and no step context is busy any more
    bool close(int item)
    {
        std::unique_lock<std::mutex> lk(mu);
        items[item].open = false;
        const bool last = --nopen == 0;
        if (last) cv.wait(lk, [&] { return !any_busy(); });
        return last;
    }
    void set_qp(int item, int qp) { std::lock_guard<std::mutex> lk(mu); items[item].qp = qp; }
    void force_idr(int item) { std::lock_guard<std::mutex> lk(mu); items[item].seq.force_idr = 1; }
    void set_idr_pic_id(int item, int next) { std::lock_guard<std::mutex> lk(mu); items[item].seq.idr_id = next & 0xFF; }
    int last_cur(int item) { std::lock_guard<std::mutex> lk(mu); return items[item].last_cur; }
    int last_layer(int item) { std::lock_guard<std::mutex> lk(mu); return items[item].last_layer; }
    int last_rband(int item) { std::lock_guard<std::mutex> lk(mu); return items[item].last_rband; }
    void last_step(int item, uint64_t* serial, int* n, int* pos, int* idr)
    {
        std::lock_guard<std::mutex> lk(mu);
        const Item& it = items[item];
        if (serial) *serial = it.step_serial;
        if (n) *n = it.step_n;
        if (pos) *pos = it.step_pos;
        if (idr) *idr = it.step_idr ? 1 : 0;
    }

    // A picture is about to be uploaded: a step that is being gathered waits (briefly) for it.  ready() runs under the lock (what
    // the upload needs and is shared, allocated once); false refuses the picture.  Returns the streams open, -1 when refused.
    template <class Ready>
    int begin_upload(Ready&& ready)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!ready()) return -1;
        uploading++;
        return nopen;
    }

    // Queue the stream's picture (uploaded: the upload begun above has ended, well or not); lead a step or wait for the one that
    // takes it.  run(HubStep&) launches the step, waits for it and answers in rc[k]; it runs without the lock.  Returns
    // false when the upload had failed (nothing was queued).
    template <class Run>
    bool encode(int item, bool uploaded, bool upload_ok, Run&& run)
    {
        std::unique_lock<std::mutex> lk(mu);
        if (uploaded) uploading--;
        if (!upload_ok) { cv.notify_all(); return false; }
        Item& it = items[item];
        it.done = false;
        const uint64_t t_q = now_us();
        queue[it.seq.next_is_idr(it.gop) ? 1 : 0].push_back(item);
        cv.notify_all();   // (a leader that is gathering counts the uploads still on their way)
        HubStep T;
        while (!it.done) {
            // lead a step if one can start: an IDR step when IDR pictures wait and the IDR context is free, else a P step
            int c = -1;
            bool idr = false;
            if (!queue[1].empty() && !busy[nctx_p]) { c = nctx_p; idr = true; }
            else if (!queue[0].empty() && !collecting)
                for (int ci = 0; ci < nctx_p && c < 0; ci++) if (!busy[ci]) c = ci;
            if (c < 0) { cv.wait(lk); continue; }
            busy[c] = true;
            if (!idr && uploading > 0 && window_us > 0) {   // pictures on their way in join this step if they make it within the window
                collecting = true;
                cv.wait_until(lk, HUB_SCHED_CLOCK::now() + std::chrono::microseconds(window_us), [&] { return uploading == 0; });
                collecting = false;
            }
            std::vector<int>& q = queue[idr ? 1 : 0];
            T.ctx = c; T.idr = idr; T.nopen = nopen;
            T.n = (int)(idr ? q.size() : std::min(q.size(), p_share()));
            for (int k = 0; k < T.n; k++) {
                Item& b = items[q[k]];
                b.seq.begin(idr);
                T.picks[k] = b.seq.pic(q[k], b.qp, idr, nrefs);
                T.rc[k] = 0;
            }
            // positions by their number of reference pictures, most first (queue order within a number): the motion search of
            // reference picture r is then one launch over the first positions, those that have it
            if (nrefs > 1) std::stable_sort(T.picks, T.picks + T.n, [](const ItemPic& a, const ItemPic& b) { return a.nref > b.nref; });
            for (int k = 0; k < T.n; k++) {
                Item& b = items[T.picks[k].item];
                b.step_serial = steps + 1; b.step_n = T.n; b.step_pos = k; b.step_idr = idr;
            }
            q.erase(q.begin(), q.begin() + T.n);
            steps++; pictures += (uint64_t)T.n; max_batch = std::max<uint64_t>(max_batch, (uint64_t)T.n);
            us_queue += now_us() - t_q;   // (the leader's own wait; the followers' is within a step of it)
            if (!q.empty()) cv.notify_all();   // what is left can start on another free context at once
            lk.unlock();
            run(T);
            lk.lock();
            for (int k = 0; k < T.n; k++) {
                Item& b = items[T.picks[k].item];
                if (T.rc[k] == 0) { b.last_cur = b.seq.cur; b.last_layer = T.picks[k].layer; b.last_rband = T.picks[k].rband; b.seq.advance(idr, nbuf, 1); }
                else b.seq.force_idr = 1;   // the picture is missing from the stream (or not to be trusted): the next one must not refer to it
                                            // (a layer-1 picture nobody refers to: one rule for both layers all the same)
                b.done = true;
            }
            busy[c] = false;
            cv.notify_all();
        }
        return true;
    }
};

}  // namespace
