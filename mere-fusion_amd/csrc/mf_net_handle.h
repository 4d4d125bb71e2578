// The mf_net handle (mf_net.hip) for the files that append ops of their own to its schedule (mf_dwpose_ops.hip).
#pragma once
#include "mf_nn.h"
#include "mf_schedule.h"

// (the Schedule member, and its graphs with it, goes before the NetStore base frees the buffers they point into)
struct mf_net : NetStore {
    int precision = MF_PREC_BF16X3, cap = 1;
    Schedule sch;                                                          // the op list and its runner (no side branches here: it never forks)
    void* scratch = nullptr;                                               // mf_net_scratch: the candidate lists of mf_s3fd_detect
    size_t scratch_bytes = 0;

    ActBuf* B(int id) { return id >= 0 && id < (int)bufs.size() ? bufs[id].get() : nullptr; }
};

#define NET_BUF(var, id) ActBuf* var = h->B(id); MF_REQUIRE(var, "net: no buffer %d", id)
