// Check of vr_devbuf_grow / vr_devbuf_grow_group / vr_devbuf_reserve (vrenderer_amd/csrc/vr_devbuf.h) with a counting allocator
// over malloc: for a single buffer and for groups of 1..15, from empty, from full and from mixed slots, with the k-th allocation
// failing for every k (and for none), and with a quiesce hook that refuses; for the reserve, with an allocator that grants
// everything, one that refuses whatever is larger than the request (the doubled size), and one that refuses everything.
//   failure: every pointer and capacity bit-identical to before, the live blocks are the blocks live before (nothing leaked,
//            nothing freed), quiesce not called (or, where it refused, called once and nothing freed but the new blocks);
//   success: every old block freed exactly once and behind quiesce, quiesce called once if an old block existed and never
//            otherwise, every slot holds a live block of the size asked for, the capacity equals the request.
//   reserve: the capacity it reaches is the policy's - the smallest of 64 KiB, 128 KiB, .. (from empty) or of twice, four times, ..
//            the old capacity that holds the request; exactly the request where that is refused; otherwise as a failure above,
//            with one allocation tried per size and quiesce never asked twice.
// Plain C++17, no GPU: g++ -std=c++17 -Wall -Werror -I vrenderer_amd/csrc tests/host/devbuf_check.cpp
#include "vr_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

static long cases = 0, failures = 0;
#define CHECK(cond) do { if (!(cond)) { failures++; std::printf("FAIL line %d: %s  [%s]\n", __LINE__, #cond, what); } } while (0)

// ---- the allocator -----------------------------------------------------------------------
static std::map<void*, size_t> live;            // block -> its size
static std::vector<void*> freed;                // every release, in order
static long alloc_calls = 0, fail_at = 0;       // the fail_at-th allocation from now fails (0: none)
static size_t refuse_above = 0;                 // every allocation larger than this fails (0: no limit)
static bool refuse_all = false;
static long quiesce_calls = 0;
static size_t frees_at_quiesce = 0;             // releases seen when quiesce ran
static int quiesce_result = 0;

static bool test_alloc(void** out, size_t bytes)
{
    if (++alloc_calls == fail_at || refuse_all || (refuse_above && bytes > refuse_above)) return false;
    *out = std::malloc(bytes ? bytes : 1);
    live[*out] = bytes;
    return true;
}
static void test_release(void* p)
{
    freed.push_back(p);
    if (live.erase(p) != 1) { failures++; std::printf("FAIL: release of a block that is not live\n"); return; }
    std::free(p);
}
static int test_quiesce() { quiesce_calls++; frees_at_quiesce = freed.size(); return quiesce_result; }
static void reset(long fail, int quiesce_rc) { freed.clear(); alloc_calls = 0; fail_at = fail; quiesce_calls = 0; frees_at_quiesce = 0; quiesce_result = quiesce_rc; }
static void* old_block(size_t bytes) { void* p = nullptr; fail_at = 0; test_alloc(&p, bytes); return p; }

// what both functions promise, given the slots before and after
template <size_t N>
static void judge(const char* what, int rc, long fail, int quiesce_rc, void* const (&before)[N], void* const (&after)[N], const size_t (&bytes)[N],
                  const std::map<void*, size_t>& live_before)
{
    cases++;
    bool any_old = false;
    for (void* p : before) any_old |= p != nullptr;
    const bool refused = fail == 0 && any_old && quiesce_rc != 0;
    if (fail != 0 || refused) {
        CHECK(rc == (refused ? quiesce_rc : kDevBufNoMemory));
        CHECK(std::memcmp(before, after, sizeof(before)) == 0);
        CHECK(live == live_before);
        CHECK(quiesce_calls == (refused ? 1 : 0));
        CHECK(alloc_calls == (refused ? (long)N : fail));                   // (stops at the first failure)
        CHECK(freed.size() == (size_t)(refused ? (long)N : fail - 1));         // (the new blocks it had obtained, nothing else)
        for (void* p : freed) CHECK(live_before.count(p) == 0);
        return;
    }
    CHECK(rc == 0);
    CHECK(alloc_calls == (long)N);
    CHECK(quiesce_calls == (any_old ? 1 : 0));
    size_t olds = 0;
    for (size_t i = 0; i < N; i++) {
        CHECK(after[i] != nullptr && live.count(after[i]) == 1 && live[after[i]] == bytes[i]);
        CHECK(live_before.count(after[i]) == 0);
        for (size_t j = 0; j < i; j++) CHECK(after[i] != after[j]);
        if (!before[i]) continue;
        olds++;
        size_t times = 0, first = 0;
        for (size_t f = 0; f < freed.size(); f++) if (freed[f] == before[i]) { if (!times) first = f; times++; }
        CHECK(times == 1);
        CHECK(first >= frees_at_quiesce);                                   // behind quiesce
        CHECK(live.count(before[i]) == 0);
    }
    CHECK(freed.size() == olds);
    CHECK(frees_at_quiesce == 0);
    CHECK(live.size() == live_before.size() - olds + N);
}

template <size_t N, size_t... I>
static int grow_group(void* (&ptr)[N], const size_t (&bytes)[N], std::index_sequence<I...>)
{
    void** const slot[N] = { &ptr[I]... };
    return vr_devbuf_grow_group(slot, bytes, test_alloc, test_release, test_quiesce);
}

// pattern: 0 = every slot empty, 1 = every slot holds a block, 2 / 3 = every other one does (even / odd slots)
template <size_t N>
static void group_cases()
{
    char what[64];
    for (int pattern = 0; pattern < 4; pattern++)
        for (int quiesce_rc = 0; quiesce_rc <= 7; quiesce_rc += 7)
            for (long fail = 0; fail <= (long)N; fail++) {
                std::snprintf(what, sizeof(what), "group N=%zu pattern=%d fail=%ld quiesce=%d", N, pattern, fail, quiesce_rc);
                void* ptr[N]; void* before[N]; size_t bytes[N];
                for (size_t i = 0; i < N; i++) {
                    const bool has = pattern == 1 || (pattern == 2 && i % 2 == 0) || (pattern == 3 && i % 2 == 1);
                    ptr[i] = has ? old_block(16 + i) : nullptr;
                    before[i] = ptr[i];
                    bytes[i] = 8 * i + (i % 3 == 0 ? 24 : 5);       // some larger than the old block, some smaller: a group replaces them all
                }
                void* bystander = old_block(3);                    // a live block that is none of the group's business
                const std::map<void*, size_t> live_before = live;
                reset(fail, quiesce_rc);
                const int rc = grow_group(ptr, bytes, std::make_index_sequence<N>());
                judge(what, rc, fail, quiesce_rc, before, ptr, bytes, live_before);
                CHECK(live.count(bystander) == 1);
                while (!live.empty()) { std::free(live.begin()->first); live.erase(live.begin()); }
            }
    if constexpr (N > 1) group_cases<N - 1>();
}

static void single_cases()
{
    char what[64];
    const size_t have[3] = { 0, 100, 4096 }, ask[6] = { 0, 1, 100, 101, 4096, 1 << 20 };
    for (size_t h : have)
        for (size_t a : ask)
            for (int quiesce_rc = 0; quiesce_rc <= 7; quiesce_rc += 7)
                for (long fail = 0; fail <= 1; fail++) {
                    std::snprintf(what, sizeof(what), "single have=%zu ask=%zu fail=%ld quiesce=%d", h, a, fail, quiesce_rc);
                    void* ptr[1] = { h ? old_block(h) : nullptr };           // (NULL, 0): growing from empty
                    void* const before[1] = { ptr[0] };
                    size_t cap = h;
                    const size_t bytes[1] = { a };
                    const std::map<void*, size_t> live_before = live;
                    reset(fail, quiesce_rc);
                    const int rc = vr_devbuf_grow(&ptr[0], &cap, a, test_alloc, test_release, test_quiesce);
                    if (a <= h) {                                            // large enough already: nothing at all happens
                        cases++;
                        CHECK(rc == 0 && alloc_calls == 0 && quiesce_calls == 0 && freed.empty());
                        CHECK(ptr[0] == before[0] && cap == h && live == live_before);
                    } else {
                        judge(what, rc, fail, quiesce_rc, before, ptr, bytes, live_before);
                        CHECK(cap == (rc == 0 ? a : h));
                    }
                    while (!live.empty()) { std::free(live.begin()->first); live.erase(live.begin()); }
                }
}

// mode: 0 = every size granted, 1 = only what is no larger than the request, 2 = nothing
static void reserve_cases()
{
    char what[80];
    const size_t have[4] = { 0, 100, 1 << 16, 3 << 16 }, ask[5] = { 1, 1 << 16, (1 << 16) + 1, 200000, 1 << 20 };
    for (size_t h : have)
        for (size_t a : ask)
            for (int quiesce_rc = 0; quiesce_rc <= 7; quiesce_rc += 7)
                for (int mode = 0; mode < 3; mode++) {
                    std::snprintf(what, sizeof(what), "reserve have=%zu ask=%zu mode=%d quiesce=%d", h, a, mode, quiesce_rc);
                    cases++;
                    void* ptr = h ? old_block(h) : nullptr;
                    void* const before = ptr;
                    size_t cap = h;
                    const std::map<void*, size_t> live_before = live;
                    reset(0, quiesce_rc);
                    refuse_above = mode == 1 ? a : 0; refuse_all = mode == 2;
                    const int rc = vr_devbuf_reserve(&ptr, &cap, a, test_alloc, test_release, test_quiesce);
                    refuse_above = 0; refuse_all = false;
                    size_t doubled = h ? h * 2 : (size_t)1 << 16;          // the policy, written out again
                    while (doubled < a) doubled *= 2;
                    const bool exact = mode == 1 && doubled > a;            // the doubled size is refused, the request granted
                    const bool refused = mode != 2 && h != 0 && quiesce_rc != 0;
                    if (a <= h) {
                        CHECK(rc == 0 && alloc_calls == 0 && quiesce_calls == 0 && freed.empty());
                        CHECK(ptr == before && cap == h && live == live_before);
                    } else if (mode == 2 || refused) {
                        CHECK(rc == (mode == 2 ? kDevBufNoMemory : quiesce_rc));
                        CHECK(ptr == before && cap == h && live == live_before);
                        CHECK(alloc_calls == (mode == 2 ? (doubled > a ? 2 : 1) : (exact ? 2 : 1)));      // one try per size, none behind a refusing quiesce
                        CHECK(quiesce_calls == (refused ? 1 : 0));
                        CHECK(freed.size() == (size_t)(refused ? 1 : 0));
                        for (void* p : freed) CHECK(live_before.count(p) == 0);
                    } else {
                        CHECK(rc == 0);
                        CHECK(cap == (exact ? a : doubled));
                        CHECK(alloc_calls == (exact ? 2 : 1));
                        CHECK(ptr != nullptr && ptr != before && live.count(ptr) == 1 && live[ptr] == cap);
                        CHECK(quiesce_calls == (h ? 1 : 0) && frees_at_quiesce == 0);
                        CHECK(freed.size() == (size_t)(h ? 1 : 0) && (!h || (freed[0] == before && live.count(before) == 0)));
                        CHECK(live.size() == live_before.size() + (h ? 0 : 1));
                    }
                    while (!live.empty()) { std::free(live.begin()->first); live.erase(live.begin()); }
                }
}

int main()
{
    single_cases();
    reserve_cases();
    group_cases<15>();
    std::printf("devbuf: %ld cases, %ld failures\n", cases, failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
