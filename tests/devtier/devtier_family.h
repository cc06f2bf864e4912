// TEST INFRASTRUCTURE: what the device tier's families share (devtier.hip, devtier_pairing.hip).  A family is a struct with
//   static Shape shape(int op)                      words per case of the operand arrays a, b, c and of the result (o == 0: unknown op)
//   static void run(int op, a, b, c, out)           one case, on the host or in a lane
// and run_family applies it to n cases: a host loop, or one launch with one lane per case in 64-lane workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../libzkp_amd/csrc/zkp_common.h"

namespace devtier {

// words per case of the three operand arrays and of the result; o == 0 marks an unknown op
struct Shape { uint32_t a, b, c, o; };

template <class T, int N> ZKP_HD inline T ld(const uint32_t* w) { T r; ZKP_UNROLL for (int i = 0; i < N; i++) r.v[i] = w[i]; return r; }
template <class T, int N> ZKP_HD inline void st(uint32_t* w, const T& x) { ZKP_UNROLL for (int i = 0; i < N; i++) w[i] = x.v[i]; }

// ------------------------------------------------------------------------------------------------ one lane per case, 64-lane blocks
template <class Case> __global__ void __launch_bounds__(64) k_devtier(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const Shape s = Case::shape(op);
    Case::run(op, a + (size_t)i * s.a, b + (size_t)i * s.b, c + (size_t)i * s.c, out + (size_t)i * s.o);
}

constexpr uint32_t MAX_CASES = 1u << 16;

template <class Case> int run_family(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) {
    const Shape s = Case::shape(op);
    if (s.o == 0 || n == 0 || n > MAX_CASES || !out || (s.a && !a) || (s.b && !b) || (s.c && !c)) return -1;
    if (!on_device) {
        for (uint32_t i = 0; i < n; i++) Case::run(op, a + (size_t)i * s.a, b + (size_t)i * s.b, c + (size_t)i * s.c, out + (size_t)i * s.o);
        return 0;
    }
    const uint32_t* host[3] = {a, b, c};
    const uint32_t words[3] = {s.a, s.b, s.c};
    uint32_t* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; k++) {
        if (!words[k]) continue;
        const size_t bytes = (size_t)n * words[k] * 4;
        e = hipMalloc((void**)&dev[k], bytes);
        if (e == hipSuccess) e = hipMemcpy(dev[k], host[k], bytes, hipMemcpyHostToDevice);
    }
    const size_t obytes = (size_t)n * s.o * 4;
    if (e == hipSuccess) e = hipMalloc((void**)&dev[3], obytes);
    if (e == hipSuccess) e = hipMemset(dev[3], 0xA5, obytes);      // a lane that stores nothing is seen
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_devtier<Case>, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, dev[0], dev[1], dev[2], dev[3]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dev[3], obytes, hipMemcpyDeviceToHost);
    for (int k = 0; k < 4; k++) if (dev[k]) (void)hipFree(dev[k]);
    return (int)e;
}

}  // namespace devtier
