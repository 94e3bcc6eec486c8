// Driver around the reference's own bilinear sampler, extras/stnbhwd/BilinearSamplerBHWD.cu, compiled unmodified for the GPU
// (oracle/reference.py builds this file into oracle/_ref/; the include below is resolved through -I <reference>/extras/stnbhwd,
// nothing of that file lives in this tree).  The entries take host pointers with the shapes of b2f_op_warp_bhwd and
// b2f_op_warp_bhwd_backward, do what the Lua module does around the native call (BilinearSamplerBHWD.lua:70 sizes the output by
// the grid, :99-102 zero both gradInputs), and call the reference's static cunn_* functions: its kernels, its launch geometry,
// its stride-argument order.  TEST INFRASTRUCTURE ONLY.
#include "BilinearSamplerBHWD.cu"

#include <cstdarg>
#include <cstring>

static THCState g_state = {0};
static int g_therror = 0;

THCState *getCutorchState(lua_State *L)
{
    (void)L;
    return &g_state;
}

void THError(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    g_therror = 1;
}

namespace {

// a contiguous B x h x w x c tensor on the device; freed with the scope
struct Dev {
    THCudaTensor t;
    hipError_t err;
    Dev(int B, int h, int w, int c) : err(hipSuccess)
    {
        t.size[0] = B; t.size[1] = h; t.size[2] = w; t.size[3] = c;
        t.stride[3] = 1; t.stride[2] = c; t.stride[1] = (long)w * c; t.stride[0] = (long)h * w * c;
        t.data = nullptr;
        err = hipMalloc((void **)&t.data, bytes());
    }
    ~Dev() { if (t.data) (void)hipFree(t.data); }
    size_t bytes() const { return sizeof(float) * (size_t)t.size[0] * t.size[1] * t.size[2] * t.size[3]; }
    hipError_t put(const float *host) { return err != hipSuccess ? err : hipMemcpy(t.data, host, bytes(), hipMemcpyHostToDevice); }
    hipError_t zero() { return err != hipSuccess ? err : hipMemset(t.data, 0, bytes()); }
    hipError_t poison() { return err != hipSuccess ? err : hipMemset(t.data, 0xff, bytes()); }   // NaN: an element left out shows
    hipError_t get(float *host) const { return hipMemcpy(host, t.data, bytes(), hipMemcpyDeviceToHost); }
    Dev(const Dev &) = delete;
    Dev &operator=(const Dev &) = delete;
};

#define REF_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

bool bad_shape(int B, int ih, int iw, int C, int gh, int gw)
{
    return B <= 0 || ih <= 0 || iw <= 0 || C <= 0 || gh <= 0 || gw <= 0 || B > 65535 || gh > 65535;
}

// after the native call: the launch error it may have reported through THError, then the kernel's own
int finish()
{
    if (g_therror) { g_therror = 0; (void)hipDeviceSynchronize(); return -2; }
    REF_TRY(hipDeviceSynchronize());
    return 0;
}

int backward(const float *img, const float *grid, const float *grad_out, int B, int ih, int iw, int C, int gh, int gw, float *grad_img,
             float *grad_grid, bool only_grid)
{
    if (!img || !grid || !grad_out || !grad_grid || (!only_grid && !grad_img) || bad_shape(B, ih, iw, C, gh, gw)) return -1;
    Dev di(B, ih, iw, C), dg(B, gh, gw, 2), dgo(B, gh, gw, C), dgg(B, gh, gw, 2);
    REF_TRY(di.put(img)); REF_TRY(dg.put(grid)); REF_TRY(dgo.put(grad_out)); REF_TRY(dgg.zero());
    lua_State L;
    memset(&L, 0, sizeof L);
    L.slot[2] = &di.t; L.slot[3] = &dg.t; L.slot[5] = &dgg.t; L.slot[6] = &dgo.t;
    g_therror = 0;
    if (only_grid) {
        cunn_BilinearSamplerBHWD_updateGradInputOnlyGrid(&L);
        const int rc = finish();
        if (rc) return rc;
    } else {
        Dev dgi(B, ih, iw, C);
        REF_TRY(dgi.zero());
        L.slot[4] = &dgi.t;
        cunn_BilinearSamplerBHWD_updateGradInput(&L);
        const int rc = finish();
        if (rc) return rc;
        REF_TRY(dgi.get(grad_img));
    }
    REF_TRY(dgg.get(grad_grid));
    return 0;
}

}  // namespace

#define REF_API extern "C" __attribute__((visibility("default")))

// img B x ih x iw x C, grid B x gh x gw x 2 (x first) -> out B x gh x gw x C; 0 or the HIP error (-1: bad arguments, -2: THError)
REF_API int ref_sampler_forward(const float *img, const float *grid, int B, int ih, int iw, int C, int gh, int gw, float *out)
{
    if (!img || !grid || !out || bad_shape(B, ih, iw, C, gh, gw)) return -1;
    Dev di(B, ih, iw, C), dg(B, gh, gw, 2), dout(B, gh, gw, C);
    REF_TRY(di.put(img)); REF_TRY(dg.put(grid)); REF_TRY(dout.poison());   // the module only resizes its output (:70)
    lua_State L;
    memset(&L, 0, sizeof L);
    L.slot[2] = &di.t; L.slot[3] = &dg.t; L.slot[4] = &dout.t;
    g_therror = 0;
    cunn_BilinearSamplerBHWD_updateOutput(&L);
    const int rc = finish();
    if (rc) return rc;
    REF_TRY(dout.get(out));
    return 0;
}

// grad_out B x gh x gw x C -> grad_img B x ih x iw x C, grad_grid B x gh x gw x 2
REF_API int ref_sampler_backward(const float *img, const float *grid, const float *grad_out, int B, int ih, int iw, int C, int gh, int gw,
                                 float *grad_img, float *grad_grid)
{
    return backward(img, grid, grad_out, B, ih, iw, C, gh, gw, grad_img, grad_grid, false);
}

// the onlyGrid instantiation: no image gradient is computed
REF_API int ref_sampler_backward_only_grid(const float *img, const float *grid, const float *grad_out, int B, int ih, int iw, int C, int gh,
                                           int gw, float *grad_grid)
{
    return backward(img, grid, grad_out, B, ih, iw, C, gh, gw, nullptr, grad_grid, true);
}
