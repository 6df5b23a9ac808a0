// staging.hpp — where the parts of one packed staging block lie: one after the other in the order they are
// taken, each on a multiple of `align` (a power of two).  Offsets only: the buffers stay with the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ygzfe {

struct BlockLayout {
    size_t align, last = 0;  // last: the end of the last part, before its padding
    size_t size() const { return (last + align - 1) & ~(align - 1); }  // every part, padded
    size_t end() const { return last; }                                // without the last part's padding
    size_t take(size_t count, size_t elem = 1) {                       // offset of a new part of count * elem bytes
        const size_t o = size();
        last = o + count * elem;
        return o;
    }
};

// the T at byte `off` of the block at `p`
template <class T>
T *at(void *p, size_t off) { return reinterpret_cast<T *>(static_cast<uint8_t *>(p) + off); }
template <class T>
const T *at(const void *p, size_t off) { return reinterpret_cast<const T *>(static_cast<const uint8_t *>(p) + off); }

}  // namespace ygzfe
