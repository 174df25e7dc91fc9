// chunk_loop.h -- host plumbing of a renderer's Chunk loop, shared by render.hip (nrf_renderer) and lerf_render.hip (nrf_lerf_renderer): the lanes (auxiliary streams
// with their fork / join events) and the feature view a one-chunk render leaves behind.  What goes on which lane and in which pieces is each renderer's own policy
// and stays in its file.  (The workspace bump allocator both use is workspace.h's.)
#pragma once

#include "common.h"
#include "workspace.h"

#include <cstdlib>
#include <mutex>

namespace nrf {

// The lanes of a Chunk loop: auxiliary streams and the fork / join events, created on first use on the device that is current then and re-created when a later call
// comes on another device.  A renderer serves one device and one caller at a time (include/nerfpp_hip.h, nrf_batchify_rays).
struct Lanes {
    static constexpr int MAX = 4;
    std::mutex mu;
    hipStream_t lane[MAX] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, done_ev[MAX] = {nullptr, nullptr, nullptr, nullptr};
    int device = -1;
    void drop()
    {
        for (auto &st : lane) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
        for (auto &e : done_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (fork_ev) { (void)hipEventDestroy(fork_ev); fork_ev = nullptr; }
        device = -1;
    }
    ~Lanes() { drop(); }
    // the first `lanes` streams with their done events, and the fork event; allow_cu_mask: the NRF_LANE_CU_MASK experiment applies to this renderer's lanes
    int acquire(int lanes, bool allow_cu_mask, hipStream_t *st, hipEvent_t *fork, hipEvent_t *done)
    {
        std::lock_guard<std::mutex> lk(mu);
        int dev = 0;
        NRF_HIP(hipGetDevice(&dev));
        if (device >= 0 && device != dev) {
            // the renderer is now used on another device: its lanes move with it (the old ones are drained and destroyed on their own device)
            (void)hipSetDevice(device);
            drop();
            NRF_HIP(hipSetDevice(dev));
        }
        for (int i = 0; i < lanes; i++) {
            if (!lane[i]) {
                // NRF_LANE_CU_MASK=1 (experiment, docs/history/profiles/round4/r4z_*): lane i of L on its own 256 / L compute units (hipExtStreamCreateWithCUMask; a contiguous bit range)
                static const int masked = [] { const char *e = getenv("NRF_LANE_CU_MASK"); return e ? atoi(e) : 0; }();
                if (allow_cu_mask && masked && lanes > 1) {
                    uint32_t bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    const int per = 256 / lanes;
                    for (int b = i * per; b < (i + 1) * per; b++) bits[b >> 5] |= 1u << (b & 31);
                    NRF_HIP(hipExtStreamCreateWithCUMask(&lane[i], 8, bits));
                } else NRF_HIP(hipStreamCreateWithFlags(&lane[i], hipStreamNonBlocking));
            }
            if (!done_ev[i]) NRF_HIP(hipEventCreateWithFlags(&done_ev[i], hipEventDisableTiming));
            st[i] = lane[i]; done[i] = done_ev[i];
        }
        if (!fork_ev) NRF_HIP(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        *fork = fork_ev;
        device = dev;
        return NRF_OK;
    }
};

// the L lanes wait for what the caller's stream `st` holds so far
static inline int fork_lanes(hipStream_t st, hipEvent_t fork, const hipStream_t *lane, int L, const char *who)
{
    bool ok = hipEventRecord(fork, st) == hipSuccess;
    for (int j = 0; j < L && ok; j++) ok = hipStreamWaitEvent(lane[j], fork, 0) == hipSuccess;
    if (ok) return NRF_OK;
    set_error("%s: forking the lanes failed", who);
    return NRF_ERR_HIP;
}

// ... and `st` waits for the lanes.  Run on every path: whatever was launched is ordered before the caller's next operation (a lane whose join failed is drained on
// the host instead); rc keeps the first error.
static inline void join_lanes(hipStream_t st, const hipStream_t *lane, const hipEvent_t *done, int L, const char *who, int &rc)
{
    for (int j = 0; j < L; j++) {
        if (hipEventRecord(done[j], lane[j]) != hipSuccess || hipStreamWaitEvent(st, done[j], 0) != hipSuccess) {
            if (rc == NRF_OK) { set_error("%s: joining the lanes failed", who); rc = NRF_ERR_HIP; }
            (void)hipStreamSynchronize(lane[j]);
        }
    }
}

// Where the last chunk left the hash features of its fine depths in the caller's workspace (nrf_renderer_last_features / nrf_lerf_renderer_last_features; the
// training backward reads them instead of encoding the fine points again): the level-major fp16 table, its column count, the keep mask by column, the merge map
// [n, sf].  Every chunk invalidates the view on entry and may set it at its end; a call that rendered several chunks drops it (the view describes ONE chunk's
// workspace).  serial: chunks rendered so far -- a caller that saw serial k and still sees k knows that no render has touched the view since.
struct FeatureView {
    const void *feats = nullptr;
    int64_t cols = 0;
    const uint8_t *keep = nullptr;
    const int32_t *src = nullptr;
    int64_t n = 0;
    int sf = 0;
    bool valid = false;
    uint64_t serial = 0;
    void begin_chunk() { valid = false; serial++; }
    void set(const void *feats_, int64_t cols_, const uint8_t *keep_, const int32_t *src_, int64_t n_, int sf_)
    {
        feats = feats_; cols = cols_; keep = keep_; src = src_; n = n_; sf = sf_; valid = true;
    }
    void drop() { valid = false; }
    // the out-parameters of the *_last_features entries (serial is optional and set either way); no_view: the caller's text for "the last call left none"
    int read(const void **feats_, int64_t *cols_, const uint8_t **keep_, const int32_t **src_, int64_t *n_, int *sf_, uint64_t *serial_, const char *no_view) const
    {
        if (serial_) *serial_ = serial;
        if (!valid) { set_error("%s", no_view); return NRF_ERR_UNSUPPORTED; }
        *feats_ = feats; *cols_ = cols; *keep_ = keep; *src_ = src; *n_ = n; *sf_ = sf;
        return NRF_OK;
    }
};

}  // namespace nrf
