// The one definition of "library-owned, per (device, stream)" (DESIGN.md section 1): a fixed table of entries keyed by (device, stream
// [, one extra word]) and the one rule by which a buffer in an entry grows.
//
// An entry is occupied because its `used` flag says so, never because a pointer in its payload is non-null: a buffer whose regrow failed
// is null with size 0 and its entry still belongs to its key.  Entries keep their address and are never given up before process exit,
// except by release() right after the claim, when the first set-up of the payload failed.
//
// Every operation wants the table's lock() held.  A caller that hands out nonces, parities or ticket bases keeps the lock until it has;
// a caller that grows a buffer keeps it across erl_slot_grow, i.e. across one hipStreamSynchronize -- growth happens a few times per
// process.  What a call does with its entry after unlocking is ordered by the entry's stream, as all work of one (device, stream) is.
//
// Deliberately NOT on this table: optim.hip's g_ra (keyed by device alone, see its comment; blocking memset + device sync), the
// measurement pools of api.cpp, the p2p.hip / comm.cpp handles and the one-off allocation in ppo_step_s3_impl.h.
#pragma once
#include <cstddef>
#include <cstdint>
#include <mutex>

template <class Payload, int Cap>
class StreamSlots {
    struct Entry {
        bool used = false;
        int device = -1;
        const void *stream = nullptr;
        int64_t extra = 0;
        Payload payload{};
    };
    Entry e_[Cap];
    std::mutex mu_;

public:
    std::unique_lock<std::mutex> lock() { return std::unique_lock<std::mutex>(mu_); }

    Payload *find(int device, const void *stream, int64_t extra = 0)
    {
        for (Entry &e : e_)
            if (e.used && e.device == device && e.stream == stream && e.extra == extra) return &e.payload;
        return nullptr;
    }

    // the key's entry, or a free one claimed for it with a value-initialised payload; nullptr: the table is full
    Payload *find_or_claim(int device, const void *stream, int64_t extra = 0)
    {
        if (Payload *p = find(device, stream, extra)) return p;
        for (Entry &e : e_)
            if (!e.used) {
                e.used = true; e.device = device; e.stream = stream; e.extra = extra;
                return &e.payload;
            }
        return nullptr;
    }

    // gives a just-claimed entry back (its set-up failed): free again, payload value-initialised
    void release(Payload *p)
    {
        for (Entry &e : e_)
            if (&e.payload == p) e = Entry{};
    }
};

#if defined(__HIPCC__)
#include "erl_common.h"

// The growth rule of a library-owned buffer: *buf holds *have bytes and must hold `need`.  Never shrinks; to grow it waits for `owner`
// (the stream whose kernels use the buffer), frees, allocates.  On any failure *buf == nullptr and *have == 0 (a block whose stream
// could not be waited for is abandoned, not freed).  `what` names the allocation in the error text.
static inline int erl_slot_grow(void **buf, size_t *have, size_t need, hipStream_t owner, const char *what)
{
    if (*have >= need) return ERL_OK;
    int rc;
    if (void *old = *buf) {
        *buf = nullptr;
        *have = 0;
        if ((rc = erl_hip_status(hipStreamSynchronize(owner), "hipStreamSynchronize"))) return rc;
        if ((rc = erl_hip_status(hipFree(old), "hipFree"))) return rc;
    }
    if ((rc = erl_hip_status(hipMalloc(buf, need), what))) *buf = nullptr;
    else *have = need;
    return rc;
}
#endif
