// ck_carve.h -- one block of memory cut into parts that each start on 16 bytes: a bump allocator over offsets.  Plain C++, no
// HIP and no context.  The kernels read the staged blocks by offset with wide loads, so every part of every block of the
// entry points (ck_stage_layout.h) is placed by this and by nothing else.
#pragma once
#include <stddef.h>

inline size_t ck_up16(size_t v) { return (v + 15) & ~(size_t)15; }

struct CkCarve {
    size_t at = 0;
    // where a part of `bytes` bytes lies; the next one starts on the next multiple of 16 behind it (a part of 0 bytes takes
    // no room and shares its offset with the next)
    size_t take(size_t bytes)
    {
        const size_t a = at;
        at = ck_up16(at + bytes);
        return a;
    }
    size_t size() const { return at; }
};
