// A ring of frame tables, for the ER-NeRF entry points whose kernels read one table entry per frame (mf_nerf_head_batch.hip, mf_nerf_frame_batch.hip,
// mf_nerf_torso_forward_batch in mf_nerf_net.hip).  A call fills the next entry's table in pinned host memory, copies it to the entry's device table on the
// caller's stream and records an event behind its last launch; the entry is written again only after that event, so a call never overwrites the table of an earlier
// call that may still be in flight, and nothing waits for the host unless as many calls as the ring has entries are.  Host only.
#pragma once
#include "mf_common.h"
#include <vector>

struct TableRing {
    // pinned staging and its device copy, `bytes` each; an event behind the last launch of the call that used the entry
    struct Entry { void *host = nullptr, *dev = nullptr; hipEvent_t done = nullptr; bool used = false; };
    std::vector<Entry> entries;
    size_t bytes = 0;                            // per entry: set by the owner before the first ensure() / acquire()
    int next = 0;
    bool ready = false;
    explicit TableRing(int depth) : entries((size_t)depth) {}
    TableRing(const TableRing&) = delete;
    ~TableRing() {
        for (Entry& e : entries) {
            if (e.done) { if (e.used) (void)hipEventSynchronize(e.done); (void)hipEventDestroy(e.done); }
            if (e.host) (void)hipHostFree(e.host);
            if (e.dev) (void)hipFree(e.dev);
        }
    }
    // allocates the ring: a create calls it to pay up front; acquire() does otherwise, for an owner whose create must touch no device
    int ensure() {
        if (ready) return MF_OK;
        for (Entry& e : entries) {
            if (!e.host) MF_HIP(hipHostMalloc(&e.host, bytes, hipHostMallocDefault));
            if (!e.dev) MF_HIP(hipMalloc(&e.dev, bytes));
            if (!e.done) MF_HIP(hipEventCreateWithFlags(&e.done, hipEventDisableTiming));
        }
        ready = true;
        return MF_OK;
    }
    // the next entry: its pinned table to fill
    int acquire(int* slot, void** tab_host) {
        if (int rc = ensure()) return rc;
        Entry& e = entries[(size_t)next];
        if (e.used) MF_HIP(hipEventSynchronize(e.done));                   // returns at once unless every entry belongs to a call in flight
        *slot = next; *tab_host = e.host;
        next = (next + 1) % (int)entries.size();
        return MF_OK;
    }
    // the table's first `n` bytes to the entry's device copy on `s`; *tab_dev is what the kernels read
    int upload(int slot, size_t n, hipStream_t s, const void** tab_dev) {
        Entry& e = entries[(size_t)slot];
        MF_HIP(hipMemcpyAsync(e.dev, e.host, n, hipMemcpyHostToDevice, s));
        e.used = true;
        *tab_dev = e.dev;
        return MF_OK;
    }
    // behind the call's last launch
    int release(int slot, hipStream_t s) { MF_HIP(hipEventRecord(entries[(size_t)slot].done, s)); return MF_OK; }
    // the three as every caller strings them: fill(T* table) writes n entries, launch(const T* device table) enqueues what reads them.  The event is recorded after a
    // failed launch too: the copy of the table is on the stream
    template <class T, class Fill, class Launch>
    int call(int n, hipStream_t s, Fill fill, Launch launch) {
        int rc, slot;
        void* host;
        const void* dev;
        if ((rc = acquire(&slot, &host))) return rc;
        fill((T*)host);
        if ((rc = upload(slot, (size_t)n * sizeof(T), s, &dev))) return rc;
        rc = launch((const T*)dev);
        const int rc2 = release(slot, s);
        return rc ? rc : rc2;
    }
};
