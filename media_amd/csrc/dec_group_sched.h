// media_amd/csrc/dec_group_sched.h -- the part of a decoder group (dec_group.h) that knows nothing of HIP: the pool of parse
// threads with its hand-out of jobs, and the rotation of the two sets of pinned picture buffers.  Plain C++, so that
// tools/dec_group_sched_harness.cpp can run it under ThreadSanitizer (tests/test_dec_group_sched.py), as hub_sched.h is.
//
// Parse jobs.  A step hands the pool one job per participating stream; job k is parse(stream[k], set).  Jobs are taken from a
// counter under the lock, first come first served, by min(jobs, threads) threads - every job is run exactly once, by one thread.  A
// step of ONE job is run by the caller itself: waking a thread for it costs more than it saves; a group of one stream - the decoder
// peer is one - starts no thread at all.  run() returns when every job of the step has finished, so a step's jobs never
// overlap the next step's, and what the jobs wrote is visible to the caller (the lock orders it).
//
// Buffer sets.  The streams parse into their slices of one SET of group-wide pinned arrays, laid [item][...], from which the step's
// uploads then run asynchronously, one transfer per array.  There are two sets: while the uploads out of one are in flight the next
// step's access units are parsed into the other.  The rotation is the group's, not each stream's - a transfer covers the slices of
// several streams, so all of a step's streams must lie in the same set.  begin_step() names the set to parse into: the one the
// last launched step did NOT use; if uploads out of it (two steps back) are still marked in flight it waits for them first through
// the caller's function.  end_step(true) marks the set in flight and makes it the last used; end_step(false) - a step in which no
// stream produced a picture - leaves everything as it was, so the same set is handed out again.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

enum { DEC_GROUP_MAX_STREAMS = 64, DEC_GROUP_MAX_THREADS = 16 };

struct DecGroupSched {
    typedef std::function<void(int stream, int set)> ParseFn;

    // ---- the pool ----
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::vector<std::thread> threads;
    bool quit = false;
    // the step in hand (all under mu)
    uint64_t gen = 0;           // changes with every step handed to the pool
    const int* streams = nullptr;
    int njobs = 0, next = 0, finished = 0, set = 0;
    const ParseFn* fn = nullptr;
    int last_threads = 0;       // threads the last step could use

    void start(int nthreads)
    {
        if (nthreads < 1) nthreads = 1;
        if (nthreads > DEC_GROUP_MAX_THREADS) nthreads = DEC_GROUP_MAX_THREADS;
        for (int i = 0; i < nthreads; i++) threads.emplace_back([this] { worker(); });
    }
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv_work.notify_all();
        for (auto& t : threads) t.join();
        threads.clear();
    }
    // run parse(streams[k], set) for k = 0 .. n - 1 and return when all have finished
    void run(const int* job_streams, int n, int job_set, const ParseFn& parse)
    {
        if (n <= 0) { last_threads = 0; return; }
        if (n == 1 || threads.empty()) {
            for (int k = 0; k < n; k++) parse(job_streams[k], job_set);
            last_threads = 1;
            return;
        }
        std::unique_lock<std::mutex> lk(mu);
        streams = job_streams; njobs = n; next = 0; finished = 0; set = job_set; fn = &parse;
        gen++;
        last_threads = n < (int)threads.size() ? n : (int)threads.size();
        lk.unlock();
        if (last_threads >= (int)threads.size()) cv_work.notify_all();
        else for (int i = 0; i < last_threads; i++) cv_work.notify_one();
        lk.lock();
        cv_done.wait(lk, [this] { return finished == njobs; });
        fn = nullptr; streams = nullptr; njobs = 0; next = 0; finished = 0;
    }

    // ---- the two buffer sets (touched by the group's caller only: a group is driven by one thread at a time) ----
    int last_set = 1;                        // the set the last launched step parsed into (the first step takes set 0)
    bool in_flight[2] = {false, false};      // uploads out of the set have been queued and not yet waited for
    int parsing = -1;                        // the set handed out by begin_step and not yet given back
    template <class Wait>
    int begin_step(Wait&& wait_uploads)      // wait_uploads(set): blocks until the uploads out of `set` have finished
    {
        const int k = last_set ^ 1;
        if (in_flight[k]) { wait_uploads(k); in_flight[k] = false; }
        parsing = k;
        return k;
    }
    void end_step(bool launched)
    {
        if (launched) { in_flight[parsing] = true; last_set = parsing; }
        parsing = -1;
    }

private:
    void worker()
    {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv_work.wait(lk, [&] { return quit || (gen != seen && next < njobs); });
            if (quit) return;
            const uint64_t g = gen;
            while (gen == g && next < njobs) {
                const int k = next++;
                const int stream = streams[k], s = set;
                const ParseFn* f = fn;
                lk.unlock();
                (*f)(stream, s);
                lk.lock();
                if (++finished == njobs) cv_done.notify_one();
            }
            seen = g;
        }
    }
};
