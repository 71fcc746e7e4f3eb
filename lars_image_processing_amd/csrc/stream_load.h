// Streaming tile loads: bytes that one workgroup reads once.  One copy of the raw-buffer loads the counting and plane-writing
// kernels use, with the cache policy as a compile-time parameter (the builtin's last argument must be an immediate).
// Loads of tables, lists and hand-over words are not streaming reads and do not belong here.
#pragma once
#include "common.h"

namespace lars {

// The cache-policy immediate of the gfx950 buffer loads, as read off the disassembly (profiles/load_policy_probe.txt):
// bit 1 = nt, bit 4 = sc1 (bit 0 would be sc0; not used for streams).
enum : int { LOAD_PLAIN = 0, LOAD_NT = 2, LOAD_SC1 = 16, LOAD_NT_SC1 = 18 };

typedef unsigned int sl_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int sl_u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned int sl_u32x4 __attribute__((ext_vector_type(4)));

template <int POLICY>
__device__ inline sl_u32x3 stream_load_b96(__amdgpu_buffer_rsrc_t rsrc, unsigned int voff, unsigned int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b96(rsrc, voff, soff, POLICY);
}
template <int POLICY>
__device__ inline sl_u32x4 stream_load_b128(__amdgpu_buffer_rsrc_t rsrc, unsigned int voff, unsigned int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, POLICY);
}
template <int POLICY>
__device__ inline sl_u32x2 stream_load_b64(__amdgpu_buffer_rsrc_t rsrc, unsigned int voff, unsigned int soff)
{
    return __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, soff, POLICY);
}

// The same choice for a tile addressed through a pointer (global loads take plain or nt only).
template <int POLICY, typename V>
__device__ inline V stream_load_ptr(const V *p)
{
    static_assert(POLICY == LOAD_PLAIN || POLICY == LOAD_NT, "pointer loads: plain or nt");
    if constexpr (POLICY == LOAD_NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// Four RGBA pixels (one 16-byte load) as the three dwords of an RGB quad; alpha is dropped.
__device__ inline sl_u32x3 rgba_quad_to_rgb(sl_u32x4 p)
{
    sl_u32x3 r;
    r.x = __builtin_amdgcn_perm(p.y, p.x, 0x04020100u);
    r.y = __builtin_amdgcn_perm(p.z, p.y, 0x05040201u);
    r.z = __builtin_amdgcn_perm(p.w, p.z, 0x06050402u);
    return r;
}

}  // namespace lars
