// What the kernels of the table loss share (b2f_tableloss.hip: test.lua:266-297; b2f_tableloss_ft.hip: the fine-tuning terms of
// README.md:89-102; b2f_tableloss_grad.hip: the gradient table of train.lua:428-468): how a thread loads and stores its pixels of a row and
// where the planes of a level lie.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace b2f {

constexpr int kLossPx = 4;   // consecutive pixels of a row per thread: one 16-byte load per plane and row

// n (1..4) samples of a row at p: one 16-byte load where the address allows -- rows of odd w are not aligned --, scalar loads
// otherwise; v[n..] is left alone
__device__ __forceinline__ void load_px(const float *p, int n, float *v)
{
    if (n == kLossPx && ((uintptr_t)p & 15) == 0) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        return;
    }
    for (int k = 0; k < kLossPx; ++k)
        if (k < n) v[k] = p[k];
}

// n (1..4) samples of a row to p: one 16-byte store where the address allows, scalar stores otherwise
__device__ __forceinline__ void store_px(float *p, int n, const float *v)
{
    if (n == kLossPx && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (int k = 0; k < kLossPx; ++k)
        if (k < n) p[k] = v[k];
}

// the planes of one level: image 0; image b lies 2 hw (f, p, o), 3 hw (iw1, iw3) or ref_stride (ref) samples further
struct LevelPtrs {
    const float *f, *p, *o, *iw1, *iw3, *ref;
    size_t ref_stride;
};

}  // namespace b2f
