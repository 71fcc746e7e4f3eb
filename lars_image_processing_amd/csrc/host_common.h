// Host-only plumbing shared by every translation unit of liblars_hip.so: status codes, the thread-local error message.
// No HIP here: host_core.cpp and tiff_codec.cpp build with a plain host compiler too (`make asan`: g++
// -fsanitize=address,undefined, the sanitizer target SURVEY.md section 5 asks for; never run on the GPU box).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "lars_hip.h"

namespace lars {

void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define LARS_TRY(expr)                \
    do {                              \
        int _s = (expr);              \
        if (_s != LARS_OK) return _s; \
    } while (0)

// workgroups of a one-dimensional grid-stride launch over n items, per_block items to a workgroup's first sweep: 1 .. 2048
inline int grid_1d(long long n, long long per_block = 256)
{
    const long long b = (n + per_block - 1) / per_block;
    return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b));
}

// p on a multiple of a (a power of two)
inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace lars
