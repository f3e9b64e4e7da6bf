// boundary.hpp -- host only: what every extern "C" entry asks of the pointers it is handed (include/rfops.h states the
// rules), and the bump counter that lays out a workspace.  Each rule once; an entry still writes `if (!...) return RF_EINVAL;`
// itself, so the order of its checks reads in the entry.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "wave.hpp"  // align256

namespace rf {

using Pointers = std::initializer_list<const void *>;

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// NULL or 8-byte aligned: an optional tensor of 64-bit elements (rf_grid_cluster's code), read and written by the element
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// no pointer is NULL
inline bool all_given(Pointers ps) {
    for (const void *p : ps)
        if (!p) return false;
    return true;
}
// every pointer is NULL or 4-byte aligned: tensors and count arrays, read and written by the word
inline bool all_aligned4(Pointers ps) {
    for (const void *p : ps)
        if (!aligned4(p)) return false;
    return true;
}
// every pointer is NULL or 16-byte aligned: optional sorted-set handles, tensors read as float4 rows
inline bool all_aligned16(Pointers ps) {
    for (const void *p : ps)
        if (!aligned16(p)) return false;
    return true;
}
// a tensor is non-NULL and 4-byte aligned; an optional tensor or count array is NULL or 4-byte aligned
inline bool tensors_ok(Pointers required, Pointers optional = {}) {
    return all_given(required) && all_aligned4(required) && all_aligned4(optional);
}
// Workspaces and sorted-set handles are read with 16-byte vector loads at offsets that are multiples of 256: the pointer the
// caller hands over must be 16-byte aligned (anything hipMalloc returns is).  Checked at the boundary -- a misaligned
// sub-allocation would otherwise be a memory fault inside a kernel.
inline bool workspace_ok(const void *w) { return w && aligned16(w); }

// One description per workspace: a function adds its sections in order and returns their offsets with `total`; the size
// query returns `total` and the entry carves the caller's buffer at the same offsets.
// add() rounds every section up to 256 bytes, so every offset is a multiple of 256 and a section of a 16-byte aligned
// workspace is 16-byte aligned for the vector loads.
struct Layout {
    size_t total = 0;
    size_t add(size_t bytes) {
        const size_t off = total;
        total += align256(bytes);
        return off;
    }
};

}  // namespace rf
