// media_amd/csrc/dev_mem.h -- DevMem: the list of device and pinned allocations of one owner (picture store / engine, stream hub,
// decoder group), and its test mode: guard regions around every block and poison in what is not zeroed by design, so that the
// suite can see a kernel's stray store and a read of memory nobody has written (tests/test_gpu_mem_guard.py; GPU AddressSanitizer
// is not an option on shared machines).
//
// The HIP calls it makes go through the eight functions of the seam `dm` below, so that this file also compiles without HIP:
// tools/dev_mem_harness.cpp defines DEV_MEM_SEAM and binds the seam to malloc / free / memset / memcpy before including it.
//
// Off (the default): no launch, no copy and no allocation differs - dev() is hipMalloc(bytes) (+ hipMemset when zeroed by design),
// pinned() is hipHostMalloc(bytes), exactly as before the mode existed.
//
// On, with guard size g (a multiple of 4096, at most 1 MiB: every alignment up to 4096 bytes that the allocator gave is kept) and
// the poison flag: a block of `bytes` is an allocation of bytes + 2 g, the caller gets base + g, and
//   - both guard regions hold the pattern  guard_byte(i), i = 0 .. g - 1 from the region's first byte (never 0, changes with i);
//   - with poison, a block that is not zeroed by design (zero == false, and every pinned block) is filled with POISON_BYTE.
// dev_bytes / pinned_bytes count the caller's bytes in either mode.  check() compares every guard with the pattern; drop() and
// free_all() check what they free and add the damage to a process-wide tally, and a line per damaged region to the file that
// MI355X_H264_MEM_GUARD_LOG names - how a run of a whole test suite under the environment variables is read at its end.
// What this cannot see: a read out of bounds, and a store that misses by more than g (a whole item or plane stride).
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#ifndef DEV_MEM_SEAM
namespace dm {
typedef hipError_t err_t;
const err_t OK = hipSuccess;
inline err_t dev_alloc(void** p, size_t n) { return hipMalloc(p, n); }
inline err_t dev_free(void* p) { return hipFree(p); }
inline err_t dev_set(void* p, int v, size_t n) { return hipMemset(p, v, n); }
inline err_t to_dev(void* d, const void* h, size_t n) { return hipMemcpy(d, h, n, hipMemcpyHostToDevice); }
inline err_t from_dev(void* h, const void* d, size_t n) { return hipMemcpy(h, d, n, hipMemcpyDeviceToHost); }
inline err_t pin_alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
inline err_t pin_free(void* p) { return hipHostFree(p); }
inline err_t sync() { return hipStreamSynchronize(nullptr); }   // (the fills above run on the null stream)
}  // namespace dm
#endif

namespace {

// for the set-up functions that hand the error on (their callers undo and translate): the call that failed, for the report
thread_local const char* t_failed_call = "";
#define DMTRY(what, call)                                              \
    do {                                                               \
        dm::err_t _r = (call);                                         \
        if (_r != dm::OK) { t_failed_call = what; return _r; }         \
    } while (0)

enum { MEM_GUARD_UNIT = 4096, MEM_GUARD_MAX = 1 << 20, POISON_BYTE = 0xCB };
inline uint8_t guard_byte(size_t i) { return (uint8_t)((i * 167u + (i >> 8) * 29u) | 1u); }

// the process-wide setting (mi355x_h264_debug_mem_guard; MI355X_H264_MEM_GUARD=<bytes>, MI355X_H264_MEM_POISON=1 give the first),
// the tally of damage found while freeing, and the pattern of the guard size in use
struct MemGuardSetting { size_t guard = 0; bool poison = false; };
struct MemGuardGlobal {
    std::mutex mu;
    MemGuardSetting cur;
    bool env_read = false;
    std::atomic<unsigned long long> tally{0};
    std::vector<uint8_t> pattern;   // guard_byte(0 .. MEM_GUARD_MAX - 1), made with the first guarded block
};
inline MemGuardGlobal& mem_guard_global() { static MemGuardGlobal g; return g; }
inline bool mem_guard_size_ok(long long g) { return g >= 0 && g <= MEM_GUARD_MAX && g % MEM_GUARD_UNIT == 0; }
inline MemGuardSetting mem_guard_setting()
{
    MemGuardGlobal& G = mem_guard_global();
    std::lock_guard<std::mutex> lk(G.mu);
    if (!G.env_read) {
        G.env_read = true;
        const char* gs = getenv("MI355X_H264_MEM_GUARD");
        const char* ps = getenv("MI355X_H264_MEM_POISON");
        const long long g = gs ? atoll(gs) : 0;
        if (g > 0 && mem_guard_size_ok(g)) { G.cur.guard = (size_t)g; G.cur.poison = ps && ps[0] == '1' && !ps[1]; }
    }
    return G.cur;
}
inline bool mem_guard_set(long long guard, bool poison)   // false: refused, nothing changes
{
    if (!mem_guard_size_ok(guard)) return false;
    (void)mem_guard_setting();   // (the environment's setting is the first, not a later one)
    MemGuardGlobal& G = mem_guard_global();
    std::lock_guard<std::mutex> lk(G.mu);
    G.cur.guard = (size_t)guard; G.cur.poison = guard > 0 && poison;
    return true;
}
inline const uint8_t* mem_guard_pattern()
{
    MemGuardGlobal& G = mem_guard_global();
    std::lock_guard<std::mutex> lk(G.mu);
    if (G.pattern.empty()) {
        G.pattern.resize(MEM_GUARD_MAX);
        for (size_t i = 0; i < (size_t)MEM_GUARD_MAX; i++) G.pattern[i] = guard_byte(i);
    }
    return G.pattern.data();
}

// one damaged guard region: offsets count from the caller's pointer (before: -g .. -1, after: bytes .. bytes + g - 1)
struct MemDamage {
    std::string name;
    bool after;
    long long first, last;
    size_t count;
    std::string line() const
    {
        char b[256];
        snprintf(b, sizeof(b), "%s %s first=%lld last=%lld bytes=%zu", name.c_str(), after ? "after" : "before", first, last, count);
        return b;
    }
};
inline void mem_guard_log(const std::vector<MemDamage>& found)
{
    const char* path = getenv("MI355X_H264_MEM_GUARD_LOG");
    if (found.empty() || !path || !*path) return;
    if (FILE* f = fopen(path, "a")) {
        for (const MemDamage& d : found) fprintf(f, "%s\n", d.line().c_str());
        fclose(f);
    }
}

// Every device or pinned allocation of an owner (store, engine, hub, decoder group) is registered where it is made and freed in one
// loop; dev_bytes / pinned_bytes: what the owner holds at the moment (the caller's bytes: guards are not counted).
struct DevMem {
    struct Block { void* p; size_t bytes; bool pinned; const char* name; };   // p: what the caller got (base + guard)
    std::vector<Block> blocks;
    size_t dev_bytes = 0, pinned_bytes = 0;
    size_t guard = 0;       // of every block of this owner; 0: the mode is off
    bool poison = false;
    // the owner is being created: the process-wide setting holds for it from here on, whatever the switch does later
    void configure() { if (blocks.empty()) { const MemGuardSetting s = mem_guard_setting(); guard = s.guard; poison = s.poison; } }

    // name: the member the block is for, as the source spells it (DM_DEV / DM_PINNED below); a literal, it is not copied
    template <class T> dm::err_t dev(T** p, size_t bytes, bool zero = false, const char* name = "?")
    {
        if (!guard) {
            DMTRY("hipMalloc", dm::dev_alloc((void**)p, bytes));
            blocks.push_back({*p, bytes, false, name});
            dev_bytes += bytes;
            if (zero) DMTRY("hipMemset", dm::dev_set(*p, 0, bytes));
            return dm::OK;
        }
        void* base = nullptr;
        DMTRY("hipMalloc", dm::dev_alloc(&base, bytes + 2 * guard));
        uint8_t* const u = (uint8_t*)base + guard;
        *p = (T*)u;
        blocks.push_back({u, bytes, false, name});
        dev_bytes += bytes;
        const uint8_t* pat = mem_guard_pattern();
        DMTRY("hipMemcpy", dm::to_dev(base, pat, guard));
        DMTRY("hipMemcpy", dm::to_dev(u + bytes, pat, guard));
        if (zero) DMTRY("hipMemset", dm::dev_set(u, 0, bytes));
        else if (poison) DMTRY("hipMemset", dm::dev_set(u, POISON_BYTE, bytes));
        DMTRY("hipStreamSynchronize", dm::sync());   // (the owners' streams do not wait for the null stream)
        return dm::OK;
    }
    template <class T> dm::err_t pinned(T** p, size_t bytes, const char* name = "?")
    {
        if (!guard) {
            DMTRY("hipHostMalloc", dm::pin_alloc((void**)p, bytes));
            blocks.push_back({*p, bytes, true, name});
            pinned_bytes += bytes;
            return dm::OK;
        }
        void* base = nullptr;
        DMTRY("hipHostMalloc", dm::pin_alloc(&base, bytes + 2 * guard));
        uint8_t* const u = (uint8_t*)base + guard;
        *p = (T*)u;
        blocks.push_back({u, bytes, true, name});
        pinned_bytes += bytes;
        const uint8_t* pat = mem_guard_pattern();
        memcpy(base, pat, guard);
        memcpy(u + bytes, pat, guard);
        if (poison) memset(u, POISON_BYTE, bytes);
        return dm::OK;
    }
    // both halves of a staging pair that comes with its first use: whichever is still missing
    template <class T> bool pair(T** d, T** h, size_t bytes, const char* dname = "?", const char* hname = "?")
    {
        if (!*d && dev(d, bytes, false, dname) != dm::OK) *d = nullptr;
        if (*d && !*h && pinned(h, bytes, hname) != dm::OK) *h = nullptr;
        return *d && *h;
    }

    // the two guard regions of one block against the pattern; what differs is appended to `found`.  false: the copy failed
    bool check_block(const Block& b, std::vector<MemDamage>& found) const
    {
        if (!guard) return true;
        const uint8_t* pat = mem_guard_pattern();
        std::vector<uint8_t> tmp;
        for (int side = 0; side < 2; side++) {
            const uint8_t* region = side ? (const uint8_t*)b.p + b.bytes : (const uint8_t*)b.p - guard;
            const uint8_t* got = region;
            if (!b.pinned) {
                tmp.resize(guard);
                if (dm::from_dev(tmp.data(), region, guard) != dm::OK) return false;
                got = tmp.data();
            }
            if (!memcmp(got, pat, guard)) continue;
            MemDamage d{b.name, side != 0, 0, 0, 0};
            const long long org = side ? (long long)b.bytes : -(long long)guard;
            for (size_t i = 0; i < guard; i++)
                if (got[i] != pat[i]) {
                    if (!d.count) d.first = org + (long long)i;
                    d.last = org + (long long)i;
                    d.count++;
                }
            found.push_back(d);
        }
        return true;
    }
    // every block's guards; the owner's work in flight has been waited for.  Returns the damaged regions appended to `found`, -1
    // when a copy failed; *regions grows by the regions looked at
    int check(std::vector<MemDamage>& found, int* regions) const
    {
        const size_t before = found.size();
        for (const Block& b : blocks) {
            if (!check_block(b, found)) return -1;
            if (guard && regions) *regions += 2;
        }
        return (int)(found.size() - before);
    }
    const Block* find(const char* name) const
    {
        for (const Block& b : blocks) if (!strcmp(b.name, name)) return &b;
        return nullptr;
    }
    // test hook: one byte of a guard region of block b set to `value` (0 .. 255), or put back to the pattern (value < 0).  offset
    // counts from the caller's pointer; anything outside the two guard regions is refused (false)
    bool poke(const Block& b, long long offset, int value) const
    {
        if (!guard || value > 255) return false;
        const long long g = (long long)guard, n = (long long)b.bytes;
        size_t i;
        if (offset >= -g && offset < 0) i = (size_t)(offset + g);
        else if (offset >= n && offset < n + g) i = (size_t)(offset - n);
        else return false;
        const int v = value < 0 ? guard_byte(i) : value;
        uint8_t* at = (uint8_t*)b.p + offset;
        if (b.pinned) { *at = (uint8_t)v; return true; }
        return dm::dev_set(at, v, 1) == dm::OK && dm::sync() == dm::OK;
    }

    void release(const Block& b)
    {
        if (guard) {
            std::vector<MemDamage> found;
            (void)check_block(b, found);
            if (!found.empty()) {
                mem_guard_global().tally.fetch_add(found.size());
                mem_guard_log(found);
            }
        }
        void* base = (uint8_t*)b.p - guard;
        if (b.pinned) (void)dm::pin_free(base); else (void)dm::dev_free(base);
    }
    // one block back ahead of the others (a staging buffer that has to grow); nothing may be using it any more
    void drop(void* p)
    {
        for (size_t i = 0; i < blocks.size(); i++)
            if (blocks[i].p == p) {
                release(blocks[i]);
                (blocks[i].pinned ? pinned_bytes : dev_bytes) -= blocks[i].bytes;
                blocks.erase(blocks.begin() + (long)i);
                return;
            }
    }
    void free_all()
    {
        for (const Block& b : blocks) release(b);
        blocks.clear(); dev_bytes = pinned_bytes = 0;
    }
};

// the call sites: the block's name is the member as the source spells it, without the owner in front of it ("e->", "h->", "g->")
inline const char* dm_name(const char* s) { const char* a = strstr(s, "->"); while (a) { s = a + 2; a = strstr(s, "->"); } return s; }
#define DM_DEV(M, member, bytes, zero) (M).dev(&(member), (bytes), (zero), dm_name(#member))
#define DM_PINNED(M, member, bytes) (M).pinned(&(member), (bytes), dm_name(#member))
#define DM_PAIR(M, d, h, bytes) (M).pair(&(d), &(h), (bytes), dm_name(#d), dm_name(#h))

}  // namespace
