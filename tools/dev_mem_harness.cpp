// tools/dev_mem_harness.cpp -- the guard mode of media_amd/csrc/dev_mem.h without HIP: the seam bound to malloc / free / memset /
// memcpy, built with -fsanitize=address,undefined and run as a program (tests/test_dev_mem_host.py).  It makes blocks of 1, 4, 4095,
// 4096 and 1 MiB + 3 bytes with guards of 4096 and 262144 bytes, poisoned and not, device and "pinned", and aborts unless: the
// caller's pointer is base + g; zeroed blocks are zero and poisoned ones are not; the totals count the caller's bytes; a clean check
// looks at 2 x blocks regions and finds nothing; a byte written at -1, -g, bytes and bytes + g - 1 is reported with the block's
// name, side and offset, one at 0 or bytes - 1 is not; poke refuses the caller's bytes; drop of a damaged block raises the tally;
// and with the switch off the sizes asked of the allocator are exactly the caller's.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I media_amd/csrc tools/dev_mem_harness.cpp
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#define DEV_MEM_SEAM
namespace dm {
typedef int err_t;
const err_t OK = 0;
std::map<void*, size_t> live;          // base -> bytes asked for
std::vector<size_t> asked;             // every size asked of the allocator, in order
int syncs = 0, sets = 0, copies = 0;
inline err_t dev_alloc(void** p, size_t n) { *p = malloc(n); if (!*p) return 1; memset(*p, 0x11, n); live[*p] = n; asked.push_back(n); return OK; }   // (never zero as it comes)
inline err_t dev_free(void* p) { if (!live.erase(p)) { fprintf(stderr, "free of a pointer the allocator never gave\n"); abort(); } free(p); return OK; }
inline err_t dev_set(void* p, int v, size_t n) { sets++; memset(p, v, n); return OK; }
inline err_t to_dev(void* d, const void* h, size_t n) { copies++; memcpy(d, h, n); return OK; }
inline err_t from_dev(void* h, const void* d, size_t n) { copies++; memcpy(h, d, n); return OK; }
inline err_t pin_alloc(void** p, size_t n) { return dev_alloc(p, n); }
inline err_t pin_free(void* p) { return dev_free(p); }
inline err_t sync() { syncs++; return OK; }
}  // namespace dm
#include "dev_mem.h"

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); abort(); } } while (0)

static const size_t SIZES[5] = {1, 4, 4095, 4096, (1u << 20) + 3};
static const char* const NAMES[5] = {"d_one", "d_four", "S.d_odd", "d_page", "d_arr[2]"};

static bool all_bytes(const uint8_t* p, size_t n, int v) { for (size_t i = 0; i < n; i++) if (p[i] != v) return false; return true; }

static void guarded(size_t g, bool poison, bool pinned)
{
    REQUIRE(mem_guard_set((long long)g, poison));
    DevMem M;
    M.configure();
    REQUIRE(M.guard == g && M.poison == poison);
    REQUIRE(mem_guard_set(0, false));   // (the owner keeps what it was created with)
    uint8_t* p[5] = {};
    size_t total = 0;
    for (int i = 0; i < 5; i++) {
        const bool zero = !pinned && (i & 1);
        const size_t n0 = dm::asked.size();
        REQUIRE((pinned ? M.pinned(&p[i], SIZES[i], NAMES[i]) : M.dev(&p[i], SIZES[i], zero, NAMES[i])) == dm::OK);
        REQUIRE(dm::asked.size() == n0 + 1 && dm::asked.back() == SIZES[i] + 2 * g);
        REQUIRE(dm::live.count(p[i] - g) == 1);                      // the caller's pointer is base + g
        REQUIRE(((uintptr_t)(p[i] - g) & 15) == ((uintptr_t)p[i] & 15));
        if (zero) REQUIRE(all_bytes(p[i], SIZES[i], 0));
        else if (poison) REQUIRE(all_bytes(p[i], SIZES[i], POISON_BYTE));
        else REQUIRE(all_bytes(p[i], SIZES[i], 0x11));               // left as it came
        total += SIZES[i];
        REQUIRE((pinned ? M.pinned_bytes : M.dev_bytes) == total && (pinned ? M.dev_bytes : M.pinned_bytes) == 0);
    }
    for (size_t i = 0; i < g; i++) REQUIRE(guard_byte(i) != 0);
    REQUIRE(guard_byte(0) != guard_byte(1) && guard_byte(5) != guard_byte(5 + 256));

    std::vector<MemDamage> found;
    int regions = 0;
    REQUIRE(M.check(found, &regions) == 0 && found.empty() && regions == 10);

    // the caller's own first and last byte: not reported
    for (int i = 0; i < 5; i++) { p[i][0] ^= 0xFF; p[i][SIZES[i] - 1] ^= 0xFF; }
    regions = 0;
    REQUIRE(M.check(found, &regions) == 0 && found.empty() && regions == 10);

    // one byte at each end of each guard, one block at a time
    const long long G = (long long)g;
    for (int i = 0; i < 5; i++) {
        const long long n = (long long)SIZES[i];
        const long long at[4] = {-1, -G, n, n + G - 1};
        for (int k = 0; k < 4; k++) {
            uint8_t* b = p[i] + at[k];
            const uint8_t was = *b;
            *b = 0;   // (the pattern is never 0)
            found.clear();
            REQUIRE(M.check(found, nullptr) == 1 && found.size() == 1);
            REQUIRE(found[0].name == NAMES[i] && found[0].after == (k >= 2) && found[0].first == at[k] && found[0].last == at[k] && found[0].count == 1);
            *b = was;
        }
        // a run: first, last and count
        for (long long o = n + 7; o < n + 19; o++) p[i][o] = 0;
        p[i][-3] = 0;
        found.clear();
        REQUIRE(M.check(found, nullptr) == 2 && found.size() == 2);
        REQUIRE(!found[0].after && found[0].first == -3 && found[0].last == -3 && found[0].count == 1);
        REQUIRE(found[1].after && found[1].first == n + 7 && found[1].last == n + 18 && found[1].count == 12);
        REQUIRE(found[1].line() == std::string(NAMES[i]) + " after first=" + std::to_string(n + 7) + " last=" + std::to_string(n + 18) + " bytes=12");
        // the poke puts the pattern back; the caller's bytes and what lies beyond the guards are refused
        const DevMem::Block* blk = M.find(NAMES[i]);
        REQUIRE(blk && blk->p == p[i]);
        for (long long o = n + 7; o < n + 19; o++) REQUIRE(M.poke(*blk, o, -1));
        REQUIRE(M.poke(*blk, -3, -1));
        REQUIRE(!M.poke(*blk, 0, 1) && !M.poke(*blk, n - 1, 1) && !M.poke(*blk, -G - 1, 1) && !M.poke(*blk, n + G, 1) && !M.poke(*blk, -1, 256));
        found.clear();
        REQUIRE(M.check(found, nullptr) == 0);
        REQUIRE(M.poke(*blk, -G, 0x5A == guard_byte(0) ? 0x5B : 0x5A) && M.check(found, nullptr) == 1 && found[0].first == -G);
        REQUIRE(M.poke(*blk, -G, -1));
        found.clear();
    }

    // a damaged block that is dropped, and one that goes with free_all: the tally
    MemGuardGlobal& GL = mem_guard_global();
    const unsigned long long t0 = GL.tally.load();
    p[2][-1] = 0;
    M.drop(p[2]);
    REQUIRE(GL.tally.load() == t0 + 1 && M.blocks.size() == 4);
    REQUIRE((pinned ? M.pinned_bytes : M.dev_bytes) == total - SIZES[2]);
    M.drop(p[0]);   // intact
    REQUIRE(GL.tally.load() == t0 + 1);
    p[4][SIZES[4]] = 0; p[4][-1] = 0;
    M.free_all();
    REQUIRE(GL.tally.load() == t0 + 3 && M.blocks.empty() && M.dev_bytes == 0 && M.pinned_bytes == 0);
    REQUIRE(M.guard == g);   // (the setting is the owner's: a geometry made again is guarded as the first was)
    REQUIRE(dm::live.empty());
}

static void off()
{
    REQUIRE(mem_guard_set(0, true));
    const MemGuardSetting s = mem_guard_setting();
    REQUIRE(s.guard == 0 && !s.poison);   // (poison without guards is no mode)
    DevMem M;
    M.configure();
    const size_t n0 = dm::asked.size();
    const int sets0 = dm::sets, copies0 = dm::copies, syncs0 = dm::syncs;
    uint8_t* p[5] = {};
    uint8_t* h = nullptr;
    for (int i = 0; i < 5; i++) REQUIRE(M.dev(&p[i], SIZES[i], i == 3, NAMES[i]) == dm::OK);
    REQUIRE(M.pinned(&h, 100, "h_x") == dm::OK);
    REQUIRE(dm::asked.size() == n0 + 6);
    for (int i = 0; i < 5; i++) { REQUIRE(dm::asked[n0 + i] == SIZES[i]); REQUIRE(dm::live.count(p[i]) == 1); }
    REQUIRE(dm::asked[n0 + 5] == 100 && dm::live.count(h) == 1);
    REQUIRE(dm::sets == sets0 + 1 && dm::copies == copies0 && dm::syncs == syncs0);   // the one block zeroed by design, nothing else
    REQUIRE(all_bytes(p[3], SIZES[3], 0) && all_bytes(p[2], SIZES[2], 0x11) && all_bytes(h, 100, 0x11));
    std::vector<MemDamage> found;
    int regions = 0;
    REQUIRE(M.check(found, &regions) == 0 && regions == 0);
    REQUIRE(!M.poke(M.blocks[0], -1, 1));
    M.drop(p[1]);
    M.free_all();
    REQUIRE(dm::copies == copies0 && dm::live.empty());
}

int main()
{
    // what the switch refuses, and that a refusal changes nothing
    REQUIRE(mem_guard_set(8192, true));
    for (long long bad : {1LL, 4095LL, 4097LL, -4096LL, (1LL << 20) + 4096, 1LL << 21})
        REQUIRE(!mem_guard_set(bad, false) && mem_guard_setting().guard == 8192 && mem_guard_setting().poison);
    REQUIRE(mem_guard_set(1 << 20, false) && mem_guard_setting().guard == (1u << 20));
    off();
    for (size_t g : {(size_t)4096, (size_t)262144})
        for (int poison = 0; poison < 2; poison++)
            for (int pinned = 0; pinned < 2; pinned++) guarded(g, poison != 0, pinned != 0);
    off();
    printf("ok dev_mem: guards 4096 and 262144, 5 sizes, poison on / off, device and pinned\n");
    return 0;
}
