// The mf_net handle (mf_net.hip) for the files that append ops of their own to its schedule (mf_dwpose_ops.hip).
#pragma once
#include "mf_conv.h"
#include "mf_schedule.h"
#include <memory>
#include <vector>

struct mf_net {
    int precision = MF_PREC_BF16X3, cap = 1;
    std::vector<std::unique_ptr<ActBuf>> bufs;
    std::vector<std::unique_ptr<ConvPlan>> plans;
    std::vector<float*> dev;
    Schedule sch;                                                          // the op list and its runner (no side branches here: it never forks)
    void* scratch = nullptr;                                               // mf_net_scratch: the candidate lists of mf_s3fd_detect
    size_t scratch_bytes = 0;

    ~mf_net() {
        sch.graph.drop_all();
        for (auto& p : plans) mf_conv_plan_destroy(p.get());
        for (auto& b : bufs) mf_actbuf_free(b.get());
        for (float* d : dev) (void)hipFree(d);
    }
    ActBuf* B(int id) { return id >= 0 && id < (int)bufs.size() ? bufs[id].get() : nullptr; }
};

#define NET_BUF(var, id) ActBuf* var = h->B(id); MF_REQUIRE(var, "net: no buffer %d", id)
