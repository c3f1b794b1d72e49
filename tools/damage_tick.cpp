// tools/damage_tick.cpp -- test helper of tests/test_gpu_damage.py (built there with g++, no HIP), tools/stream_tick.cpp for damage
// calls: hands ONE host I420 picture of each of n streams to the stream hub from n native threads that leave a gate together, each
// through the ordinary call (mode 0) or the damage call with its own rectangles (mode 1; n_rects may be the detect sentinel).  The
// entry points come as function pointers; nothing here knows the library.
#include <cstdint>
#include <pthread.h>
#include <vector>

extern "C" {

typedef int (*encode_host_fn)(void*, const uint8_t*, int, const uint8_t*, int, const uint8_t*, int, uint8_t**, uint32_t*, int*);
typedef int (*encode_damage_fn)(void*, const uint8_t*, int, const uint8_t*, int, const uint8_t*, int, const void*, int, uint8_t**, uint32_t*, int*);

// in: stream, pic (tight I420 in host memory), w, h, mode, rects / n_rects; out: rc, out / len (valid until the stream's next call), frame_type
struct DamageTickJob { void* stream; const uint8_t* pic; int32_t w, h, mode, n_rects; const void* rects; int32_t rc; uint8_t* out; uint32_t len; int32_t frame_type; };

}

namespace {
struct Gate { pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER; pthread_cond_t cv = PTHREAD_COND_INITIALIZER; int state = 0; };   // 1: go, 2: give up
struct Arg { DamageTickJob* job; encode_host_fn host; encode_damage_fn dmg; Gate* gate; };

void* work(void* p)
{
    const Arg& a = *(const Arg*)p;
    DamageTickJob& j = *a.job;
    const size_t ysz = (size_t)j.w * j.h;
    int ft = 0;
    pthread_mutex_lock(&a.gate->mu);
    while (a.gate->state == 0) pthread_cond_wait(&a.gate->cv, &a.gate->mu);
    const bool go = a.gate->state == 1;
    pthread_mutex_unlock(&a.gate->mu);
    if (!go) return nullptr;
    const uint8_t* u = j.pic + ysz, * v = u + ysz / 4;
    if (j.mode) j.rc = a.dmg(j.stream, j.pic, j.w, u, j.w / 2, v, j.w / 2, j.rects, j.n_rects, &j.out, &j.len, &ft);
    else j.rc = a.host(j.stream, j.pic, j.w, u, j.w / 2, v, j.w / 2, &j.out, &j.len, &ft);
    j.frame_type = ft;
    return nullptr;
}
}  // namespace

// 0, or -1 when the threads could not be started (no job has run then)
extern "C" int damage_tick(encode_host_fn host, encode_damage_fn dmg, DamageTickJob* jobs, int n)
{
    if (n <= 0) return 0;
    Gate gate;
    std::vector<Arg> args((size_t)n);
    std::vector<pthread_t> th((size_t)n);
    int started = 0;
    for (; started < n; started++) {
        args[started] = Arg{&jobs[started], host, dmg, &gate};
        if (pthread_create(&th[started], nullptr, work, &args[started]) != 0) break;
    }
    pthread_mutex_lock(&gate.mu);
    gate.state = started == n ? 1 : 2;   // every thread sleeps at the gate by now or finds it open: they leave it together
    pthread_cond_broadcast(&gate.cv);
    pthread_mutex_unlock(&gate.mu);
    for (int k = 0; k < started; k++) pthread_join(th[k], nullptr);
    return started == n ? 0 : -1;
}
