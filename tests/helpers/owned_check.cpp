// owned_check.cpp -- the ownership types of nerfpp_amd/csrc/owned.h on the host, without a GPU and without a HIP library: Buf over a counting fake Mem, Scratch over
// counting fakes of nrf::scratch_take / scratch_give, and the early-return macros over fakes of the three HIP calls they name.  Exit status 0: every check held;
// otherwise the line of the first one that did not.  Built and run by tests/test_owned_host.py:
//   c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I<rocm>/include -Iinclude -Inerfpp_amd/csrc tests/helpers/owned_check.cpp
#include "owned.h"

#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

// ---- fakes -------------------------------------------------------------------------------------------------------------------------------------------------------
static int g_allocs = 0, g_releases = 0, g_live = 0, g_double = 0;
static bool g_fail_alloc = false;
static std::vector<void *> g_released;

struct CountingMem {
    static constexpr const char *call = "CountingMem::alloc";
    static hipError_t alloc(void **p, size_t bytes)
    {
        if (g_fail_alloc) return hipErrorOutOfMemory;
        *p = malloc(bytes);
        g_allocs++; g_live++;
        return hipSuccess;
    }
    static void release(void *p, size_t)
    {
        for (void *q : g_released) if (q == p) g_double++;          // (freed addresses are kept, never handed to free(): no address comes back while the program runs)
        g_released.push_back(p);
        g_releases++; g_live--;
    }
};
using TestBuf = nrf::Buf<CountingMem>;

static int g_busy = 0, g_takes = 0;
static hipError_t g_last_error = hipSuccess;
static char g_block[64];

namespace nrf {
void set_error(const char *, ...) {}
void device_bytes_add(int64_t) {}
hipError_t scratch_take(void **out, size_t, hipStream_t) { *out = g_block; g_busy++; g_takes++; return hipSuccess; }
hipError_t scratch_give(void *p, hipStream_t) { if (p != g_block) return hipErrorInvalidValue; g_busy--; return hipSuccess; }
}  // namespace nrf
extern "C" const char *hipGetErrorString(hipError_t) { return "fake"; }
extern "C" hipError_t hipGetLastError(void) { const hipError_t e = g_last_error; g_last_error = hipSuccess; return e; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "owned_check.cpp:%d: %s\n", __LINE__, #cond); return __LINE__ & 0x7f ? __LINE__ & 0x7f : 1; } } while (0)

// ---- functions that leave early while they hold a Scratch ----------------------------------------------------------------------------------------------------------
static int fails() { return NRF_ERR_UNSUPPORTED; }
static int leave_by_hip(hipError_t e) { nrf::Scratch s; NRF_TRY(s.take(16, nullptr)); NRF_HIP(e); return NRF_OK; }
static int leave_by_try() { nrf::Scratch s; NRF_TRY(s.take(16, nullptr)); NRF_TRY(fails()); return NRF_OK; }
static int leave_by_launch_check(hipError_t e) { nrf::Scratch s; NRF_TRY(s.take(16, nullptr)); g_last_error = e; NRF_LAUNCH_CHECK(); return NRF_OK; }

static int run()
{
    // move construction and move assignment leave one owner
    {
        TestBuf a;
        CHECK(a.resize(32) == NRF_OK && a && a.bytes() == 32);
        void *p = a.as<void>();
        TestBuf b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b.as<void>() == p && b.bytes() == 32);
        TestBuf c;
        CHECK(c.resize(8) == NRF_OK);
        c = std::move(b);                                   // c's own block is released, b's moves in
        CHECK(!b && c.as<void>() == p && g_releases == 1 && g_live == 1);
        TestBuf &same = c;
        c = std::move(same);                                // self-assignment keeps it
        CHECK(c.as<void>() == p && g_live == 1);
    }
    CHECK(g_allocs == 2 && g_releases == 2 && g_live == 0 && g_double == 0);

    // a vector of 1 000 owners grown by push_back, then cleared
    {
        std::vector<TestBuf> v;
        std::vector<void *> at;
        for (int i = 0; i < 1000; i++) {
            TestBuf b;
            CHECK(b.resize(4 + i % 7) == NRF_OK);
            at.push_back(b.as<void>());
            v.push_back(std::move(b));
        }
        CHECK(g_live == 1000 && g_releases == 2);           // growing the vector moved the owners: nothing released, nothing copied
        for (int i = 0; i < 1000; i++) CHECK(v[i].as<void>() == at[i]);
        v.clear();
    }
    CHECK(g_allocs == 1002 && g_releases == 1002 && g_live == 0 && g_double == 0);

    // resize
    {
        TestBuf a;
        CHECK(a.resize(64) == NRF_OK);
        void *p = a.as<void>();
        const int r0 = g_releases;
        CHECK(a.resize(64) == NRF_OK && a.as<void>() == p && g_releases == r0 && g_allocs == 1003);          // the same size: the same block
        CHECK(a.resize(65) == NRF_OK && a.bytes() == 65 && g_releases == r0 + 1 && g_allocs == 1004);        // another size: the old block released exactly once
        CHECK(g_released.back() == p);
        g_fail_alloc = true;
        CHECK(a.resize(66) == NRF_ERR_HIP && !a && a.bytes() == 0 && g_releases == r0 + 2);                  // alloc fails: empty, the error returned ...
        CHECK(a.resize(66) == NRF_ERR_HIP && !a && g_releases == r0 + 2);
        g_fail_alloc = false;
        a.reset();
        CHECK(g_releases == r0 + 2);                                                                         // ... and nothing left to release again
        CHECK(a.resize(0) == NRF_OK && !a);
    }
    CHECK(g_live == 0 && g_double == 0 && g_allocs == g_releases);

    // Scratch: every way out gives the block back
    CHECK(leave_by_hip(hipErrorInvalidValue) == NRF_ERR_HIP && g_busy == 0);
    CHECK(leave_by_try() == NRF_ERR_UNSUPPORTED && g_busy == 0);
    CHECK(leave_by_launch_check(hipErrorLaunchFailure) == NRF_ERR_HIP && g_busy == 0);
    CHECK(leave_by_hip(hipSuccess) == NRF_OK && leave_by_launch_check(hipSuccess) == NRF_OK && g_busy == 0);
    CHECK(g_takes == 5);
    {
        nrf::Scratch s;
        CHECK(!s && s.take(1, nullptr) == NRF_OK && s && s.as<char>() == g_block && g_busy == 1);
        CHECK(s.take(2, nullptr) == NRF_OK && g_busy == 1);                                                  // a second take gives the first back
    }
    CHECK(g_busy == 0);
    return 0;
}

int main()
{
    const int rc = run();
    for (void *p : g_released) free(p);
    if (rc == 0) puts("owned_check: ok");
    return rc;
}
