// filter_copy.hip -- the yardstick of tools/filter_bench.py: a float4 copy kernel (read n bytes, write n bytes), timed by
// HIP events in the process that times the filter kernels.  An in-place pass over n bytes moves the same 2 n bytes.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC tools/filter_copy.hip -o build_ab/libfilter_copy.so
#include <hip/hip_runtime.h>
#include <stdint.h>

__global__ __launch_bounds__(256) void copy16_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, uint64_t n16)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// copies `bytes` (a multiple of 16) `iters` times after three warm-up launches; ms[k] = launch k by HIP events -> 0, or -1
extern "C" int filter_copy_ms(uint64_t bytes, int iters, float *ms)
{
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0, e1;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) return -1;
    if (hipMemset(a, 0x5A, bytes) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1;
    const uint64_t n16 = bytes / 16;
    const uint32_t grid = (uint32_t)((n16 + 255) / 256 < 256 * 32 ? (n16 + 255) / 256 : 256 * 32);
    int rc = 0;
    for (int k = -3; k < iters && rc == 0; k++) {
        (void)hipEventRecord(e0, nullptr);
        hipLaunchKernelGGL(copy16_kernel, dim3(grid), dim3(256), 0, nullptr, (const float4 *)a, (float4 *)b, n16);
        (void)hipEventRecord(e1, nullptr);
        if (hipEventSynchronize(e1) != hipSuccess) rc = -1;
        float t = 0;
        if (rc == 0 && hipEventElapsedTime(&t, e0, e1) != hipSuccess) rc = -1;
        if (k >= 0) ms[k] = t;
    }
    (void)hipEventDestroy(e0), (void)hipEventDestroy(e1);
    (void)hipFree(a), (void)hipFree(b);
    return rc;
}
