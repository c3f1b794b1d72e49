// tools/dec_group_sched_harness.cpp -- the HIP-free part of a decoder group (media_amd/csrc/dec_group_sched.h: hand-out of parse
// jobs to the pool, rotation of the two buffer sets) alone, under a sanitizer:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=thread -I media_amd/csrc tools/dec_group_sched_harness.cpp -o /tmp/dec_group_sched_harness
// usage: dec_group_sched_harness [steps] [seed]
// 8 pool threads, 12 streams, random participation.  A "parse" writes the stream's slice of the set it is given; an "upload" is a
// thread that reads the slices a little later and then reports itself done, as the copy engine does behind an event.  Checked on
// the way: every job of every step is run exactly once, never two at a time for one stream, a set is never handed out (or written)
// while its uploads are marked in flight, and what the upload reads is what that step's parse wrote.  Ends with "ok ..." or aborts
// with the rule that broke.  Run by tests/test_dec_group_sched.py.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "dec_group_sched.h"

#define RULE(cond, ...) do { if (!(cond)) { fprintf(stderr, "rule broken: " __VA_ARGS__); fprintf(stderr, "\n"); abort(); } } while (0)

namespace {
enum { THREADS = 8, STREAMS = 12 };
DecGroupSched S;
long g_slice[2][STREAMS];              // what the parse of step n writes: n * 100 + stream (plain memory: the sanitizer watches it)
std::atomic<int> g_uploading[2];       // an upload out of the set is running
std::atomic<int> g_in_parse[STREAMS];
std::atomic<long> g_parsed{0};
int g_runs[STREAMS];                   // jobs run for the stream in the step in hand (each written by the one thread that has the job)
std::thread g_upload[2];
}  // namespace

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 400;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    S.start(THREADS);
    long expect_parsed = 0, launched = 0;
    for (int n = 1; n <= steps; n++) {
        int jobs[STREAMS], nj = 0;
        const unsigned mode = rng() % 8;
        for (int i = 0; i < STREAMS; i++)
            if (mode == 0 ? i == (int)(rng() % STREAMS) && nj == 0 : mode == 1 ? true : rng() % 3 != 0) jobs[nj++] = i;
        const int k = S.begin_step([&](int set) { g_upload[set].join(); });   // (the event wait)
        RULE(k == 0 || k == 1, "set %d", k);
        RULE(g_uploading[k].load() == 0 && !S.in_flight[k], "step %d: set %d handed out while its uploads are in flight", n, k);
        for (int i = 0; i < STREAMS; i++) g_runs[i] = 0;
        const DecGroupSched::ParseFn parse = [&](int stream, int set) {
            RULE(set == k, "job with set %d in a step of set %d", set, k);
            RULE(g_in_parse[stream].fetch_add(1) == 0, "stream %d parsed by two threads at once", stream);
            RULE(g_uploading[set].load() == 0, "stream %d parses into set %d while it is being uploaded", stream, set);
            g_slice[set][stream] = (long)n * 100 + stream;
            g_runs[stream]++;
            if ((stream + n) % 3 == 0) std::this_thread::sleep_for(std::chrono::microseconds(30));
            g_parsed++;
            g_in_parse[stream]--;
        };
        S.run(jobs, nj, k, parse);
        expect_parsed += nj;
        RULE(g_parsed.load() == expect_parsed, "step %d: %ld jobs run, %ld handed in", n, g_parsed.load(), expect_parsed);
        for (int i = 0; i < STREAMS; i++) {
            bool in = false;
            for (int j = 0; j < nj; j++) in |= jobs[j] == i;
            RULE(g_runs[i] == (in ? 1 : 0), "step %d: stream %d parsed %d times", n, i, g_runs[i]);
        }
        RULE(nj == 0 || (S.last_threads >= 1 && S.last_threads <= std::min(nj, (int)THREADS)), "threads used %d for %d jobs", S.last_threads, nj);
        const bool launch = nj > 0 && rng() % 8 != 0;   // (a step whose pictures were all refused launches nothing)
        if (launch) {
            launched++;
            g_uploading[k].store(1);
            std::vector<int> mine(jobs, jobs + nj);
            g_upload[k] = std::thread([k, n, mine] {
                std::this_thread::sleep_for(std::chrono::microseconds(150));
                for (int i : mine) RULE(g_slice[k][i] == (long)n * 100 + i, "the upload of step %d read another step's slice of stream %d", n, i);
                g_uploading[k].store(0);
            });
        }
        S.end_step(launch);
        RULE(S.in_flight[k] == launch || (!launch && S.in_flight[k] == false), "in-flight mark of set %d", k);
    }
    for (auto& t : g_upload) if (t.joinable()) t.join();
    S.stop();
    printf("ok %d steps, %ld launched, %ld jobs\n", steps, launched, g_parsed.load());
    return 0;
}
