// workspace.h -- the one rule of the caller-owned workspaces: every workspace has ONE layout function, a sequence of Bump::take calls in a fixed order that fills a
// plain struct of pointers.  Run on a measuring Bump it yields the byte count (the *_workspace_bytes twins of the C ABI), run on the caller's buffer it yields the
// pointers; no second formula restates it.  Nested workspaces call the inner layout or size function, and a region shared by alternatives is the largest measure.
#pragma once

#include "common.h"

namespace nrf {

struct Bump {
    char *base = nullptr;          // null: measuring (take returns null and only `off` moves)
    size_t off = 0, cap = SIZE_MAX;
    Bump() = default;                                                                   // measuring mode
    Bump(void *b, size_t c) : base(static_cast<char *>(b)), cap(c) {}                    // checked mode: a caller's buffer and what the caller said it holds
    template <class T> T *take(size_t count)
    {
        off = align_up(off, 256);
        const size_t at = off;
        off += count * sizeof(T);
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    bool ok() const { return off <= cap; }                    // checked mode: every piece taken so far lies inside the buffer (pointers are used only after this holds)
    size_t bytes() const { return align_up(off, 256); }       // what a size function reports
};

// the byte count of a layout: layout(Bump &) run on a measuring Bump
template <class Layout> static inline size_t measure(Layout &&layout)
{
    Bump b;
    layout(b);
    return b.bytes();
}

// the workspace check of an entry, before its first launch: the caller's buffer holds what the size function reports (`need`) and the layout carved from it fits
static inline int ws_check(const Bump &b, size_t need, const char *who)
{
    if (b.cap >= need && b.ok()) return NRF_OK;
    set_error("%s: workspace %zu < %zu bytes", who, b.cap, need > b.off ? need : b.off);
    return NRF_ERR_WORKSPACE;
}

}  // namespace nrf
