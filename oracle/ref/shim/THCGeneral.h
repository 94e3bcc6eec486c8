/* Stand-in for cutorch's "THCGeneral.h" / THCTensor.h, for compiling the reference's extras/stnbhwd/BilinearSamplerBHWD.cu
 * with hipcc (oracle/reference.py).  Only what that file uses: a four-dimensional float tensor with sizes, strides and a
 * device pointer, the current stream (the null stream), THError, and the CUDA runtime names mapped to their HIP ones. */
#ifndef B2F_REF_SHIM_THCGENERAL_H
#define B2F_REF_SHIM_THCGENERAL_H

#include <hip/hip_runtime.h>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString
#define cudaStream_t hipStream_t

struct THCState {
    hipStream_t stream;
};

struct THCudaTensor {
    long size[4];
    long stride[4];
    float *data;
};

static inline float *THCudaTensor_data(THCState *state, const THCudaTensor *t) { (void)state; return t->data; }
static inline long THCudaTensor_stride(THCState *state, const THCudaTensor *t, int dim) { (void)state; return t->stride[dim]; }
static inline long THCudaTensor_size(THCState *state, const THCudaTensor *t, int dim) { (void)state; return t->size[dim]; }
static inline hipStream_t THCState_getCurrentStream(THCState *state) { return state->stream; }

/* defined by the driver: it records the failure, the entry returns it */
void THError(const char *fmt, ...);

#endif
