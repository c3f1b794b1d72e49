// tools/hub_sched_harness.cpp -- the stream hub's scheduling (media_amd/csrc/hub_sched.h) alone, host only, under a sanitizer:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -I media_amd/csrc tools/hub_sched_harness.cpp -o /tmp/hub_sched_harness
//   (or -fsanitize=address,undefined -fno-sanitize-recover=undefined)
// usage: hub_sched_harness [rounds] [seed]
// 64 threads open streams on one scheduler, hand it pictures, force IDR pictures (their own and, unasked, each other's), change
// QPs and close again.  The step is a short sleep that fails now and then.  Every rule the hub relies on is checked on the way;
// the run ends with "ok ..." or aborts with the rule that broke.  Run by tests/test_hub_sched.py.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>

// (a steady_clock deadline waits through pthread_cond_clockwait, which gcc 11's ThreadSanitizer does not intercept: it loses track
// of the mutex.  The library keeps steady_clock.)
#define HUB_SCHED_CLOCK std::chrono::system_clock
#include "hub_sched.h"

#define RULE(cond, ...) do { if (!(cond)) { fprintf(stderr, "rule broken: " __VA_ARGS__); fprintf(stderr, "\n"); abort(); } } while (0)

namespace {

enum { THREADS = 64, GOP = 6, NCTX_P = 2 };

HubSched S;
std::mutex g_open_mu;                 // opens and closes are serialised, as the library's are
std::atomic<int> g_in_step{0};        // steps running
std::atomic<long> g_steps{0}, g_failed{0}, g_idr{0};
// The harness's own count of open streams, as a log: entry k = the count after the k-th open or close, written under g_open_mu
// BEFORE the scheduler is told.  With n entries published the scheduler's count is entry n - 1 or, while the call is on its way,
// n - 2; so the count a step was gathered with is one of the entries from two before the leader came in to the last one now.
std::vector<int> g_open_log;          // (sized in main: never reallocated)
std::atomic<long> g_open_n{1};
void log_open(int delta) { const long n = g_open_n.load(); g_open_log[n] = g_open_log[n - 1] + delta; g_open_n.store(n + 1); }

// what the harness knows of the stream in slot `item` (the slot's owner writes before it queues, the step's leader reads and
// writes while the owner waits: ordered by the scheduler's lock, which is part of what ThreadSanitizer checks)
struct Track {
    long submitted = 0, finished = 0;   // pictures handed in / run by a step
    bool must_be_idr = false;           // first picture, own force-IDR, or the last one failed
    bool failed = false;                // the step's answer for the picture in flight
    int in_gop = 0;
} g_track[HUB_MAX_ITEMS];

// log_from: entries of g_open_log published when the step's leader came in with its picture
void fake_step(HubStep& T, std::mt19937& rng, long log_from)
{
    g_in_step++;
    g_steps++;
    bool counted = false;
    for (long k = std::max(0L, log_from - 2), n = g_open_n.load(); k < n; k++) counted = counted || g_open_log[k] == T.nopen;
    RULE(counted, "a step gathered with %d streams open, which the harness never had open meanwhile", T.nopen);
    const int share = std::max(1, (T.nopen + NCTX_P) / (NCTX_P + 1));   // the rule as the hub states it, worked out here
    RULE(T.n >= 1 && T.n <= T.nopen && (T.idr || T.n <= share), "a step of %d pictures with %d streams open (share %d)", T.n, T.nopen, share);
    RULE(T.idr ? T.ctx == NCTX_P : T.ctx < NCTX_P, "picture type and context do not match");
    std::this_thread::sleep_for(std::chrono::microseconds(20 + rng() % 80));
    const bool all_fail = rng() % 64 == 0;
    for (int k = 0; k < T.n; k++) {
        const ItemPic& p = T.picks[k];
        Track& t = g_track[p.item];
        for (int j = 0; j < k; j++) RULE(T.picks[j].item != p.item, "stream %d twice in one step", p.item);
        RULE(t.finished + 1 == t.submitted, "stream %d: picture %ld run while %ld were handed in", p.item, t.finished + 1, t.submitted);
        // one picture type per step, and the type is the one the stream's state asks for
        RULE(!t.must_be_idr || T.idr, "stream %d: a P picture where an IDR picture was due", p.item);
        RULE(T.idr ? p.frame_num == 0 : p.frame_num == t.in_gop, "stream %d: frame_num %d in a %s step, %d pictures into the GOP", p.item, p.frame_num, T.idr ? "IDR" : "P", t.in_gop);
        RULE(T.idr || t.in_gop < GOP, "stream %d: GOP longer than %d", p.item, GOP);
        RULE(p.cur >= 0 && p.cur < S.nbuf, "ring slot");
        // the picture's number of reference pictures: those coded since the stream's IDR, never one from before it (a failed picture
        // is followed by an IDR picture); a step's positions are ordered by it, most first
        RULE(p.nref == (T.idr ? 0 : std::min(S.nrefs, t.in_gop)), "stream %d: %d reference pictures, %d pictures into the GOP", p.item, p.nref, t.in_gop);
        RULE(k == 0 || T.picks[k - 1].nref >= p.nref, "position %d has more reference pictures than the one before it", k);
        t.finished++;
        t.failed = all_fail || rng() % 16 == 0;
        T.rc[k] = t.failed ? 1 : 0;
        if (T.idr) { g_idr++; t.in_gop = 0; }
        if (t.failed) g_failed++; else t.in_gop++;
    }
    g_in_step--;
}

void worker(int id, int rounds, unsigned seed)
{
    std::mt19937 rng(seed * 1000003u + (unsigned)id);
    for (int r = 0; r < rounds; r++) {
        int item;
        {
            std::lock_guard<std::mutex> gl(g_open_mu);
            log_open(+1);
            item = S.open(20 + (int)(rng() % 30), GOP);
            RULE(item >= 0, "no room for stream");
            g_track[item] = Track();
            g_track[item].must_be_idr = true;
        }
        Track& t = g_track[item];
        const int pictures = 1 + (int)(rng() % 12);
        for (int i = 0; i < pictures; i++) {
            if (rng() % 8 == 0) { S.force_idr(item); t.must_be_idr = true; }
            if (rng() % 8 == 0) S.set_qp(item, 20 + (int)(rng() % 30));
            if (rng() % 16 == 0) S.force_idr((int)(rng() % HUB_MAX_ITEMS));   // someone else's, at any moment (it may also be closed)
            if (rng() % 32 == 0) S.set_idr_pic_id(item, (int)(rng() % 256));
            const bool upload = rng() % 2 == 0, upload_ok = !upload || rng() % 32 != 0;
            if (upload) {
                RULE(S.begin_upload([] { return true; }) >= 1, "upload refused");
                std::this_thread::sleep_for(std::chrono::microseconds(rng() % 30));
            }
            if (upload_ok) t.submitted++;
            const long log_from = g_open_n.load();
            const bool queued = S.encode(item, upload, upload_ok, [&](HubStep& T) { fake_step(T, rng, log_from); });
            RULE(queued == upload_ok, "a failed upload was queued");
            if (!queued) continue;
            RULE(t.finished == t.submitted, "stream %d: encode returned with %ld of %ld pictures run", item, t.finished, t.submitted);
            t.must_be_idr = t.failed;   // after a failed step the stream's next picture is an IDR picture
        }
        {
            std::lock_guard<std::mutex> gl(g_open_mu);
            log_open(-1);
            if (S.close(item)) RULE(g_in_step.load() == 0 && !S.any_busy(), "the last close returned with a step in flight");
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 20;
    const unsigned seed = argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
    S.cap = HUB_MAX_ITEMS; S.nctx_p = NCTX_P; S.window_us = 50;
    S.nrefs = seed % 2 == 0 ? 3 : 1; S.nbuf = S.nrefs + 1;   // even seeds: streams that search three reference pictures
    g_open_log.assign((size_t)THREADS * rounds * 2 + 1, 0);
    std::vector<std::thread> th;
    for (int i = 0; i < THREADS; i++) th.emplace_back(worker, i, rounds, seed);
    for (auto& t : th) t.join();
    RULE(S.nopen == 0 && S.uploading == 0 && S.queue[0].empty() && S.queue[1].empty() && !S.any_busy(), "the scheduler is not idle at the end");
    RULE((long)S.steps == g_steps.load(), "steps counted %llu, run %ld", (unsigned long long)S.steps, g_steps.load());
    printf("ok %llu pictures in %llu steps (largest %llu), %ld IDR, %ld failed\n", (unsigned long long)S.pictures, (unsigned long long)S.steps,
           (unsigned long long)S.max_batch, g_idr.load(), g_failed.load());
    return 0;
}
