// Part of libnellie_hip.so (gfx950): included by nellie_hip.hip, see include/nellie_amd.h for the C-ABI.
// =================================================================================================
// kernels: dtype conversion
// =================================================================================================
template <typename T>
__global__ void convert_kernel(const T *__restrict__ src, float *__restrict__ dst, i64 n) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (float)src[i];
}

template <typename T>
__global__ void intensity_mask_kernel(const T *__restrict__ orig, float *__restrict__ frangi, double thresh, i64 n) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        // frangi * mask with mask bool: False -> +0.0 * x (keeps numpy's signed zero / nan semantics simple: x finite >= 0)
        if (!((double)orig[i] > thresh)) frangi[i] = frangi[i] * 0.0f;
    }
}

// The same against an integer threshold of the image's own 64-bit type, compared as integers: beyond 2^53 the conversion to
// float64 above rounds, and numpy compares a 64-bit integer array with an integer exactly.
template <typename T>
__global__ void intensity_mask_int_kernel(const T *__restrict__ orig, float *__restrict__ frangi, T thresh, i64 n) {
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (!(orig[i] > thresh)) frangi[i] = frangi[i] * 0.0f;
    }
}
