// Growing a device buffer: allocate the new block first, give the old one up only once the new one exists.  Plain C++17: no
// HIP, no library types - a CPU program walks every failure position with a counting allocator (tests/host/devbuf_check.cpp).
// The library's allocate function is vr_dev_alloc (vr_host.hip); vr_internal.h wraps the two functions below around it.
//
//   alloc(void** out, size_t bytes) -> bool     a new block, or false (then *out is not looked at)
//   release(void* block)                        gives a block back
//   quiesce() -> int                            0 once nothing in flight can still touch the old blocks (the call sites'
//                                               stream synchronisations); called at most once, in front of the first release
//                                               and only if there is an old block; its non-zero result ends the call
//
// All three return 0, kDevBufNoMemory, or what quiesce returned; unless they return 0, every pointer and capacity is what it was
// and no block has been gained or lost.  During a growth the old and the new blocks exist side by side.
#pragma once

#include <stddef.h>

constexpr int kDevBufNoMemory = -1;

// N buffers to N sizes, all or nothing: every slot gets a new block of its size, whatever it held.
template <size_t N, class Alloc, class Release, class Quiesce>
int vr_devbuf_grow_group(void** const (&slot)[N], const size_t (&bytes)[N], Alloc&& alloc, Release&& release, Quiesce&& quiesce)
{
    void* fresh[N];
    int rc = 0;
    size_t got = 0;
    while (got < N && alloc(&fresh[got], bytes[got])) got++;
    if (got < N) rc = kDevBufNoMemory;
    else {
        bool old = false;
        for (void** s : slot) old |= *s != nullptr;
        if (old) rc = quiesce();
    }
    if (rc) { while (got > 0) release(fresh[--got]); return rc; }
    for (size_t i = 0; i < N; i++) {
        if (*slot[i]) release(*slot[i]);
        *slot[i] = fresh[i];
    }
    return 0;
}

// One buffer to at least `bytes`: nothing happens if it holds that much already.
template <class Alloc, class Release, class Quiesce>
int vr_devbuf_grow(void** ptr, size_t* capacity, size_t bytes, Alloc&& alloc, Release&& release, Quiesce&& quiesce)
{
    if (bytes <= *capacity) return 0;
    void** const slot[1] = { ptr };
    const size_t want[1] = { bytes };
    const int rc = vr_devbuf_grow_group(slot, want, alloc, release, quiesce);
    if (!rc) *capacity = bytes;
    return rc;
}

// One buffer that only ever grows, to at least `bytes`: from 64 KiB by doubling, and to exactly `bytes` where the allocator refuses
// the doubled size.  (quiesce runs at most once: a refused allocation never reaches it.)
template <class Alloc, class Release, class Quiesce>
int vr_devbuf_reserve(void** ptr, size_t* capacity, size_t bytes, Alloc&& alloc, Release&& release, Quiesce&& quiesce)
{
    if (bytes <= *capacity) return 0;
    size_t want = *capacity ? *capacity * 2 : (size_t)1 << 16;
    while (want < bytes) want *= 2;
    int rc = vr_devbuf_grow(ptr, capacity, want, alloc, release, quiesce);
    if (rc == kDevBufNoMemory && want > bytes) rc = vr_devbuf_grow(ptr, capacity, bytes, alloc, release, quiesce);
    return rc;
}
